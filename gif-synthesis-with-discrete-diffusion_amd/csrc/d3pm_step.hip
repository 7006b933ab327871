// Fused D3PM reverse step: log_softmax x2 -> classifier-free mix -> q_posterior -> Gumbel arg-max.
//
// One wave64 owns one token position; the K(+1)-wide categorical lives in registers
// (lane owns quads k = 4*lane + 256*j), every reduction over classes is a wave reduction.
// HBM-bound by design: algorithmic traffic = the two logit rows (2*K*4 B) per position.
//
// Mirrors the reference op-for-op in fp32 (diffusion_transformer.py:220-283, :354-359); the
// reference's fp64 log_softmax (:231) is matched by accumulating the exp-sum and taking its log in fp64.
#include <stdlib.h>

#include "common.hpp"
#include "d3pm_rows.hpp"

namespace gsdd {

// FULL: K == 256 * J, every register slot holds a class (no validity selects).  DBG: the posterior / x0 test hooks
// are compiled in; the production instantiation has none, so the unrolled class loops are single basic blocks.
// Everything that depends only on the position (token, timestep, schedule row, which register slot holds class x_t)
// is wave-uniform: the wave index goes through readfirstlane so that the compiler keeps it in SGPRs, and the
// "k == x_t" special case becomes a scalar branch on j plus one lane compare instead of a compare+select per class.
// OCC = waves per SIMD the register budget is sized for: 3 -> 168 VGPRs, 2 -> 256.  At K = 4096 (J = 16) the two 64-register
// rows plus the temporaries of the unrolled class loops need ~180: with OCC = 3 the compiler parks 8 of them in scratch memory
// (2 KB written per position, 131 MB per launch at B*L = 65536 -- the WRITE_SIZE of profiles/r1_pmc_traffic.csv); OCC = 2 has none.
// TRUNC: top-r truncation of the guided row (truncate_row, d3pm_rows.hpp) between the guidance mix and the posterior.  It is a
// kernel family of its own (d3pm_step_trunc_kernel): the plain kernels compile the body with TRUNC = false, instruction for
// instruction what they were before the option existed.
// KNOWN: positions whose clean token is given (gsdd_step_desc.known / x_known / known_mode).  One wave owns one position, so
// known[pos] is wave-uniform: it is read through the scalar pos and branched on before the first logits load.  A known position reads
// neither logit row nor x_t and never touches x0 / xu: it keeps the three values of q(x_{t'-1} | x_0 = x_known) and walks the draw's
// register slots with the draw's Philox counters (known_row_draw, d3pm_rows.hpp); hold mode is the token store alone.  Every other
// position falls through to the code below unchanged.  Kernel families of their own again (d3pm_step_known_kernel,
// d3pm_step_known_trunc_kernel): with KNOWN = false nothing of this is compiled.
template <int J, bool FULL, bool DBG, bool TRUNC, bool KNOWN = false>
__device__ __forceinline__ void d3pm_step_body(const gsdd_step_desc& d, const SchedPtrs& sp) {
    const int lane = threadIdx.x & 63;
    const int64_t pos = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pos >= (int64_t)d.B * d.L) return;
    const int b = (int)(pos / d.L), l = (int)(pos % d.L);
    const int K = d.K;
    const float NEG = -INFINITY;

    if (KNOWN) {
        if (__builtin_amdgcn_readfirstlane((int)d.known[pos]) != 0) {       // scalar branch: the whole wave takes it or none of it
            const int xk = __builtin_amdgcn_readfirstlane((int)d.x_known[pos]);
            int win = xk;
            if (d.known_mode == 0) {    // renoise: x_{t'-1} ~ q(. | x_0 = x_known), the level t' - 1 wrapped modulo T + 1 (index T: x_known itself)
                const int64_t t_in = d.t_dev[b];
                const int64_t t = t_in > d.post_skip ? t_in - d.post_skip : t_in;
                const int64_t tp = (t - 1 + (d.T + 1)) % (d.T + 1);
                const float pca = sp.p[4][tp], pcb = sp.p[5][tp], pcc = sp.p[6][tp], p1mcc = sp.p[7][tp];
                win = known_row_draw<J, FULL>(xk, lae(0.f + pca, pcb), lae(LOG_ZERO + pca, pcb), lae(LOG_ZERO + p1mcc, pcc), lane, K,
                                              d.seed, (uint32_t)d.stream_dev[0], (uint64_t)(d.row0 + pos));
            }
            if (lane == 0) d.tok_out[pos] = win;
            return;
        }
    }

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
    if (TRUNC) truncate_row<J, FULL>(x0, d.trunc_rate, lane, K);
    if (DBG && d.x0_dbg != nullptr) {
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * lane + 256 * j + e;
                if (k < K) d.x0_dbg[((int64_t)b * (K + 1) + k) * d.L + l] = x0[j][e];
            }
        if (lane == 0) d.x0_dbg[((int64_t)b * (K + 1) + K) * d.L + l] = -70.f;
    }

    // ---- q_posterior (:251-283), at t' = t - post_skip for t > post_skip (skip-step sampling, :700-704; wave-uniform)
    const int64_t t_in = d.t_dev[b];
    const int64_t t = t_in > d.post_skip ? t_in - d.post_skip : t_in;
    const StepSched s = load_sched(sp.p, t, d.T);
    const int xt = (int)d.tok_in[pos];
    const bool masked = (xt == K);
    // class x_t sits in register slot [xj][xe] of lane xl (for x_t = [MASK] that slot does not exist or is invalid,
    // and the "hit" constants equal the "miss" ones, so no case distinction is needed below)
    const int xj = xt >> 8, xl = (xt >> 2) & 63, xe = xt & 3;
    const bool mine = (lane == xl);
    const float qt_miss = masked ? s.lcc : lae(LOG_ZERO + s.lca, s.lcb);
    const float qt_hit = masked ? s.lcc : lae(0.f + s.lca, s.lcb);
    const float q1_miss = masked ? s.lc : lae(LOG_ZERO + s.la, s.lb);
    const float q1_hit = masked ? s.lc : lae(0.f + s.la, s.lb);
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const bool valid = FULL || (4 * lane + 256 * j) < K;
        if (j == xj) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x0[j][e] = valid ? (x0[j][e] - ((mine && e == xe) ? qt_hit : qt_miss)) : NEG;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x0[j][e] = valid ? (x0[j][e] - qt_miss) : NEG;
        }
    }
    const float S = wave_logsumexp<J, !FULL>(x0, LOG_ZERO, true);
    float best = NEG;
    int best_k = 0;
    const uint32_t kp4 = (uint32_t)((K + 1 + 3) / 4);
    const uint32_t stream_id = (uint32_t)d.stream_dev[0];
    const uint64_t grow = (uint64_t)(d.row0 + pos);
    auto draw = [&](int j, int e, float log_q1, float u) {
        const int k = 4 * lane + 256 * j + e;
        const float qn = x0[j][e] - S;
        const float o = clamp70(lae(qn + s.pca, s.pcb) + log_q1 + S);
        if (DBG && d.post_dbg != nullptr) d.post_dbg[((int64_t)b * (K + 1) + k) * d.L + l] = o;
        const float v = gumbel(u) + o;
        if (v > best) { best = v; best_k = k; }
    };
    // one register slot's four classes
#define GSDD_STEP_DRAW_SLOT(j)                                                                                       \
    do {                                                                                                             \
        const int k0 = 4 * lane + 256 * (j);                                                                         \
        if (FULL || k0 < K) {                                                                                        \
            const float4 u4 = philox_uniform4(d.seed, stream_id, grow, kp4, (uint32_t)(k0 >> 2));                    \
            const float u[4] = {u4.x, u4.y, u4.z, u4.w};                                                             \
            if ((j) == xj) {                                                                                         \
                _Pragma("unroll")                                                                                    \
                for (int e = 0; e < 4; ++e) draw((j), e, (mine && e == xe) ? q1_hit : q1_miss, u[e]);                \
            } else {                                                                                                 \
                _Pragma("unroll")                                                                                    \
                for (int e = 0; e < 4; ++e) draw((j), e, q1_miss, u[e]);                                             \
            }                                                                                                        \
        }                                                                                                            \
    } while (0)
    // KNOWN at J = 32: two loops of 16 slots.  As one loop of 32 the body passes the size up to which the compiler unrolls a loop in
    // full; it then unrolls by 16 and indexes x0 with the run-time j of the loop that is left, and x0 lives in scratch memory (528
    // bytes per lane).  The families with known positions have no scratch; every other family keeps its single loop.
    constexpr int JH = (KNOWN && J > 16) ? J / 2 : J;
#pragma unroll
    for (int j = 0; j < JH; ++j) GSDD_STEP_DRAW_SLOT(j);
    if constexpr (JH < J) {
#pragma unroll
        for (int j = JH; j < J; ++j) GSDD_STEP_DRAW_SLOT(j);
    }
#undef GSDD_STEP_DRAW_SLOT
    if (lane == ((K >> 2) & 63)) {  // the [MASK] class k = K (K % 4 == 0 -> word 0 of quad K/4)
        const float4 u4 = philox_uniform4(d.seed, stream_id, grow, kp4, (uint32_t)(K >> 2));
        const float qn = LOG_ZERO - S;
        const float log_q1 = masked ? 0.f : LOG_ZERO;
        const float o = clamp70(lae(qn + s.p1mcc, s.pcc) + log_q1 + S);
        if (DBG && d.post_dbg != nullptr) d.post_dbg[((int64_t)b * (K + 1) + K) * d.L + l] = o;
        const float v = gumbel(u4.x) + o;
        if (v > best) { best = v; best_k = K; }
    }
    const int win = wave_argmax(best, best_k);
    if (lane == 0) d.tok_out[pos] = win;
}

template <int J, bool FULL, bool DBG, int OCC = 3>
__global__ __launch_bounds__(256, OCC) void d3pm_step_kernel(gsdd_step_desc d, SchedPtrs sp) {
    d3pm_step_body<J, FULL, DBG, false>(d, sp);
}

// the truncated family: two waves per SIMD throughout (the exponentials of the row take the 64 registers xu leaves)
template <int J, bool FULL, bool DBG>
__global__ __launch_bounds__(256, 2) void d3pm_step_trunc_kernel(gsdd_step_desc d, SchedPtrs sp) {
    d3pm_step_body<J, FULL, DBG, true>(d, sp);
}

// the families with known positions: no test hooks; the register budget that leaves the unknown positions' rows in registers
// (two waves per SIMD at J = 16 as in the production plain kernel, one at J = 32: 512 registers, the spill space is AGPRs)
template <int J, bool FULL>
__global__ __launch_bounds__(256, J >= 32 ? 1 : (J >= 16 ? 2 : 3)) void d3pm_step_known_kernel(gsdd_step_desc d, SchedPtrs sp) {
    d3pm_step_body<J, FULL, false, false, true>(d, sp);
}

template <int J, bool FULL>
__global__ __launch_bounds__(256, J >= 32 ? 1 : 2) void d3pm_step_known_trunc_kernel(gsdd_step_desc d, SchedPtrs sp) {
    d3pm_step_body<J, FULL, false, true, true>(d, sp);
}

// q_sample (:361-366): x_t ~ Gumbel-argmax(q_pred(onehot(x0), t))
__global__ __launch_bounds__(256) void d3pm_q_sample_kernel(const int64_t* x0, int64_t* xt, int B, int L, int K, int T,
                                                            SchedPtrs sp, const int64_t* t_dev, uint64_t seed,
                                                            const int64_t* stream_dev, int64_t row0) {
    const int lane = threadIdx.x & 63;
    const int64_t pos = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pos >= (int64_t)B * L) return;
    const int b = (int)(pos / L);
    const int64_t t = (t_dev[b] + (T + 1)) % (T + 1);
    const float lca = sp.p[4][t], lcb = sp.p[5][t], lcc = sp.p[6][t], l1mcc = sp.p[7][t];
    const int64_t tok = x0[pos];
    const float hit = lae(0.f + lca, lcb), miss = lae(LOG_ZERO + lca, lcb);
    const float mval = lae((tok == K ? 0.f : LOG_ZERO) + l1mcc, lcc);
    const uint32_t kp4 = (uint32_t)((K + 1 + 3) / 4);
    const uint32_t stream_id = (uint32_t)stream_dev[0];
    const uint64_t grow = (uint64_t)(row0 + pos);
    float best = -INFINITY;
    int best_k = 0;
    for (int k0 = 4 * lane; k0 <= K; k0 += 256) {
        const float4 u4 = philox_uniform4(seed, stream_id, grow, kp4, (uint32_t)(k0 >> 2));
        const float u[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = k0 + e;
            if (k <= K) {
                const float lp = (k == K) ? mval : (k == tok ? hit : miss);
                const float v = gumbel(u[e]) + lp;
                if (v > best) { best = v; best_k = k; }
            }
        }
    }
    const int win = wave_argmax(best, best_k);
    if (lane == 0) xt[pos] = win;
}

__global__ void advance_kernel(int64_t* t_dev, int B, int64_t dt, int64_t* stream_dev, int64_t ds) {
    const int i = threadIdx.x + blockIdx.x * blockDim.x;
    if (t_dev != nullptr && i < B) t_dev[i] += dt;
    if (stream_dev != nullptr && i == 0) stream_dev[0] += ds;
}

__global__ void advance_floor_kernel(int64_t* t_dev, int B, int64_t dt, int64_t t_min, int64_t* stream_dev, int64_t ds) {
    const int i = threadIdx.x + blockIdx.x * blockDim.x;
    if (t_dev != nullptr && i < B) t_dev[i] = t_dev[i] + dt > t_min ? t_dev[i] + dt : t_min;
    if (stream_dev != nullptr && i == 0) stream_dev[0] += ds;
}

__global__ void philox_uniform_kernel(uint64_t seed, uint32_t stream_id, int64_t row0, int64_t n_rows, int n_cols,
                                      float* out) {
    const uint32_t kp4 = (uint32_t)((n_cols + 3) / 4);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows * (int64_t)kp4) return;
    const int64_t r = i / kp4;
    const uint32_t c4 = (uint32_t)(i % kp4);
    const float4 u4 = philox_uniform4(seed, stream_id, (uint64_t)(row0 + r), kp4, c4);
    const float u[4] = {u4.x, u4.y, u4.z, u4.w};
    for (int e = 0; e < 4; ++e) {
        const int c = (int)c4 * 4 + e;
        if (c < n_cols) out[r * n_cols + c] = u[e];
    }
}


// ------------------------------------------------------------------------------------------------------------
// Training objective, forward value (diffusion_transformer.py:391-457): per position
//   log_x0_recon = predict_start(logits)                      (:231-236)
//   log_model    = q_posterior(log_x0_recon, onehot(x_t), t)   (:251-283)
//   log_true     = q_posterior(onehot(x_0),  onehot(x_t), t)
//   kl = sum_k exp(log_true)(log_true - log_model) ; nll = -sum_k exp(onehot(x_0)) log_model ;
//   kl_aux = sum_{k<K} exp(onehot(x_0)) (onehot(x_0) - log_x0_recon)
// written per position; x0_recon / x_{t-1}-recon arg-max tokens for pred_data and the acc/keep statistics.
struct TrainArgs {
    const float* logits;      // [B*L][K]
    const int64_t* x0;
    const int64_t* xt;
    const int64_t* t_dev;
    int B, L, K, T;
    float mw_mask, mw_other;  // mask_weight
    float* kl; float* nll; float* aux;       // [B*L]
    int64_t* x0_recon; int64_t* xt1_recon;   // [B*L]
    float* probs;             // optional [B][K+1][L] = exp(log_model)
};

// (two waves per SIMD: left to itself the compiler interleaves so many classes of the unrolled loops that it needs 256 VGPRs plus
// AGPR spill space, i.e. one wave per SIMD with nothing to cover its transcendentals' latency)
// FULL: K == 256 J, every register slot holds a class: no validity predicates (each `k < K` otherwise becomes an exec-mask region
// around its class: 245 s_and_saveexec + 291 branches per position in the K = 4096 instantiation).
template <int J, bool FULL = false>
__global__ __launch_bounds__(256, 2) void d3pm_train_loss_kernel(TrainArgs d, SchedPtrs sp) {
    const int lane = threadIdx.x & 63;
    const int64_t pos = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pos >= (int64_t)d.B * d.L) return;
    const int b = (int)(pos / d.L), l = (int)(pos % d.L);
    const int K = d.K;
    const float NEG = -INFINITY;
    float xr[J][4];
    const float* row = d.logits + pos * (int64_t)K;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = 4 * lane + 256 * j;
        if (FULL || k < K) {
            const float4 v = *reinterpret_cast<const float4*>(row + k);
            xr[j][0] = v.x; xr[j][1] = v.y; xr[j][2] = v.z; xr[j][3] = v.w;
        } else {
            xr[j][0] = xr[j][1] = xr[j][2] = xr[j][3] = NEG;
        }
    }
    log_softmax_clamp<J>(xr);                       // log_x0_recon rows k < K; row K is -70
    const int64_t t = d.t_dev[b];
    const StepSched s = load_sched(sp.p, t, d.T);
    const int xt = (int)d.xt[pos], x0 = (int)d.x0[pos];       // (32-bit: the per-class compares are half-rate 64-bit ones otherwise)
    const bool masked = (xt == K);
    const float qt_hit = lae(0.f + s.lca, s.lcb), qt_miss = lae(LOG_ZERO + s.lca, s.lcb);
    const float q1_hit = lae(0.f + s.la, s.lb), q1_miss = lae(LOG_ZERO + s.la, s.lb);
    // As in d3pm_train_bwd_kernel: the position is wave-uniform, the two special classes (k = x_t, k = x_0) sit in register quads
    // xj / x0j, every other quad runs on scalar constants behind a scalar branch; no second 64-register array (q = x - log_qt is
    // recomputed: one subtraction).
    const int xj = masked ? -1 : (xt >> 8), x0j = x0 >> 8;
    const float qt_c = masked ? s.lcc : qt_miss, q1_c = masked ? s.lc : q1_miss;
    const float E30 = expf(LOG_ZERO);               // exp(log-onehot "zero") as the reference computes it
    const float s_pca = s.pca, s_pcb = s.pcb, s_p1mcc = s.p1mcc, s_pcc = s.pcc;
    auto for_classes = [&](auto f) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            if (j == xj || j == x0j) {                                                  // scalar branch
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 4 * lane + 256 * j + e;
                    if (FULL || k < K) {
                        const bool hit = !masked && k == xt, tru = k == x0;
                        f(j, e, k, hit ? qt_hit : qt_c, hit ? q1_hit : q1_c, tru ? 0.f : LOG_ZERO, tru ? 1.f : E30);
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 4 * lane + 256 * j + e;
                    if (FULL || k < K) f(j, e, k, qt_c, q1_c, LOG_ZERO, E30);
                }
            }
        }
    };
    // pass 1: the two normalisers S_m (model) and S_t (true); arg-max of log_x0_recon (row K = -70 competes)
    float mxm = LOG_ZERO, mxt = LOG_ZERO;            // include the [MASK] row (= LOG_ZERO) in both maxima
    float best0 = NEG; int best0_k = 0;
    for_classes([&](int j, int e, int k, float log_qt, float, float lx0, float) {
        if (xr[j][e] > best0) { best0 = xr[j][e]; best0_k = k; }
        mxm = fmaxf(mxm, xr[j][e] - log_qt);
        mxt = fmaxf(mxt, lx0 - log_qt);
    });
    if (lane == 0 && -70.f > best0) { best0 = -70.f; best0_k = K; }     // first-max rule across the wave: wave_argmax
    const int x0rec = wave_argmax(best0, best0_k);
    mxm = wave_max(mxm); mxt = wave_max(mxt);
    float sem = 0.f, set = 0.f;
    for_classes([&](int j, int e, int, float log_qt, float, float lx0, float) {
        sem += exp_term((xr[j][e] - log_qt) - mxm);                                      // terms of sums: see exp_term
        set += exp_term((lx0 - log_qt) - mxt);
    });
    sem = wave_sum(sem) + expf(LOG_ZERO - mxm);
    set = wave_sum(set) + expf(LOG_ZERO - mxt);
    const float Sm = mxm + logf(sem), St = mxt + logf(set);
    // pass 2: posteriors, KL / NLL / aux partial sums, arg-max of log_model
    float kl = 0.f, nll = 0.f, aux = 0.f;
    float bestm = NEG; int bestm_k = 0;
    for_classes([&](int j, int e, int k, float log_qt, float log_q1, float lx0, float w0) {
        const float lm = clamp70(lae(((xr[j][e] - log_qt) - Sm) + s_pca, s_pcb) + log_q1 + Sm);
        const float ltr = clamp70(lae(((lx0 - log_qt) - St) + s_pca, s_pcb) + log_q1 + St);
        kl += exp_le0(ltr) * (ltr - lm);
        nll += w0 * lm;
        aux += w0 * (lx0 - xr[j][e]);
        if (lm > bestm) { bestm = lm; bestm_k = k; }
        if (d.probs != nullptr) d.probs[((int64_t)b * (K + 1) + k) * d.L + l] = exp_le0(lm);
    });
    kl = wave_sum(kl); nll = wave_sum(nll); aux = wave_sum(aux);
    {   // the [MASK] class row
        const float log_q1K = masked ? 0.f : LOG_ZERO;
        const float lmK = clamp70(lae((LOG_ZERO - Sm) + s_p1mcc, s_pcc) + log_q1K + Sm);
        const float ltK = clamp70(lae((LOG_ZERO - St) + s_p1mcc, s_pcc) + log_q1K + St);
        kl += expf(ltK) * (ltK - lmK);
        nll += (x0 == K ? 1.f : E30) * lmK;
        if (lane == 0) {
            if (lmK > bestm) { bestm = lmK; bestm_k = K; }
            if (d.probs != nullptr) d.probs[((int64_t)b * (K + 1) + K) * d.L + l] = expf(lmK);
        }
    }
    const int xt1 = wave_argmax(bestm, bestm_k);
    if (lane == 0) {
        const float mw = masked ? d.mw_mask : d.mw_other;
        d.kl[pos] = kl * mw;
        d.nll[pos] = -nll;
        d.aux[pos] = aux * mw;
        d.x0_recon[pos] = x0rec;
        d.xt1_recon[pos] = xt1;
    }
}

// per-sample reductions + the scalar tail of _train_loss / forward (:425-457, :548): one workgroup
struct TrainFinArgs {
    const float* kl; const float* nll; const float* aux;
    const int64_t* x0; const int64_t* xt; const int64_t* x0_recon; const int64_t* xt1_recon;
    const int64_t* t_dev; const float* pt;
    int B, L, T;
    float aux_weight; int adaptive;
    float* Lt_history; float* Lt_count;
    float* loss;              // [1]
    float* per_sample;        // [B][4]: kl_loss, vb_loss, acc rate, keep rate
};

__global__ __launch_bounds__(256) void d3pm_train_finalize_kernel(TrainFinArgs a) {
    __shared__ float red[4][256];
    __shared__ float vb_all[1024];
    const int tid = threadIdx.x;
    for (int b = 0; b < a.B; ++b) {
        float kl = 0.f, nll = 0.f, aux = 0.f, same0 = 0.f, same1 = 0.f;
        for (int l = tid; l < a.L; l += 256) {
            const int64_t p = (int64_t)b * a.L + l;
            kl += a.kl[p]; nll += a.nll[p]; aux += a.aux[p];
            same0 += (a.x0_recon[p] == a.x0[p]) ? 1.f : 0.f;
            same1 += (a.xt1_recon[p] == a.xt[p]) ? 1.f : 0.f;
        }
        // block sums: wave shuffles, then the four wave totals through LDS (two barriers per sample instead of forty-five)
        float vals[5] = {wave_sum(kl), wave_sum(nll), wave_sum(aux), wave_sum(same0), wave_sum(same1)};
        float tot[5];
        if ((tid & 63) == 0)
            for (int q = 0; q < 5; ++q) red[0][(tid >> 6) * 8 + q] = vals[q];
        __syncthreads();
        for (int q = 0; q < 5; ++q) tot[q] = (red[0][q] + red[0][8 + q]) + (red[0][16 + q] + red[0][24 + q]);
        __syncthreads();
        if (tid == 0) {
            const int64_t t = a.t_dev[b];
            const float m0 = (t == 0) ? 1.f : 0.f;
            const float kl_loss = m0 * tot[1] + (1.f - m0) * tot[0];
            float vb = kl_loss / a.pt[b];
            if (a.aux_weight != 0.f) {
                const float kl_aux_loss = m0 * tot[1] + (1.f - m0) * tot[2];
                const float w = a.adaptive ? ((1.f - (float)t / (float)a.T) + 1.0f) : 1.0f;
                vb += w * a.aux_weight * kl_aux_loss / a.pt[b];
            }
            // Lt_history.scatter_(t, 0.1*Lt2 + 0.9*prev) ; Lt_count.scatter_add_(t, 1)   (:432-436; sample order)
            const float lt2 = kl_loss * kl_loss;
            a.Lt_history[t] = 0.1f * lt2 + 0.9f * a.Lt_history[t];
            a.Lt_count[t] += 1.f;
            a.per_sample[4 * b + 0] = kl_loss;
            a.per_sample[4 * b + 1] = vb;
            a.per_sample[4 * b + 2] = tot[3] / (float)a.L;
            a.per_sample[4 * b + 3] = tot[4] / (float)a.L;
            vb_all[b] = vb;
        }
        __syncthreads();
    }
    if (tid == 0) {
        float sum = 0.f;
        for (int b = 0; b < a.B; ++b) sum += vb_all[b];
        a.loss[0] = sum / ((float)a.B * (float)a.L);
    }
}

// ------------------------------------------------------------------------------------------------------------
// Gradient of the training objective w.r.t. the denoiser logits (backward of predict_start -> q_posterior -> KL / NLL /
// aux KL, diffusion_transformer.py:391-457).  Per position, with G_c = dL/d log_model_c = -(g_kl exp(log_true_c) + g_nll w0_c):
//   lm = clamp(e + lq1 + S), e = lae(qn + alpha, beta), qn = q - S, S = lse(q), q_k = r_k - lqt_k, r = clamp(log_softmax(x))
// g_* are the per-sample weights of the three sums in loss = sum_b vb_b / (B L).
struct TrainBwdArgs {
    const float* logits; const int64_t* x0; const int64_t* xt; const int64_t* t_dev; const float* pt;
    int B, L, K, T;
    float mw_mask, mw_other, aux_weight; int adaptive;
    float* dlogits;
    float* kl; float* nll; float* aux; int64_t* x0_recon; int64_t* xt1_recon;      // LOSS = true: the forward kernel's outputs too
};

// LOSS = true (gsdd_d3pm_train_loss_grad): the same pass also leaves what d3pm_train_loss_kernel computes -- the per-position KL /
// NLL / auxiliary-KL sums and the two arg-max tokens, by the same operations in the same order (bit-identical values) -- so the
// training step reads the (B L, K) logits once instead of twice and evaluates the posteriors once (1.7 ms of a 67 ms step at bs 16).
template <int J, bool LOSS = false, bool FULL = false>
__global__ __launch_bounds__(256, 2) void d3pm_train_bwd_kernel(TrainBwdArgs d, SchedPtrs sp) {
    const int lane = threadIdx.x & 63;
    const int64_t pos = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pos >= (int64_t)d.B * d.L) return;
    const int b = (int)(pos / d.L);
    const int K = d.K;
    const float NEG = -INFINITY;
    float a[J][4];                                  // unclamped log_softmax
    const float* row = d.logits + pos * (int64_t)K;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = 4 * lane + 256 * j;
        if (FULL || k < K) {
            const float4 v = *reinterpret_cast<const float4*>(row + k);
            a[j][0] = v.x; a[j][1] = v.y; a[j][2] = v.z; a[j][3] = v.w;
        } else {
            a[j][0] = a[j][1] = a[j][2] = a[j][3] = NEG;
        }
    }
    {   // log_softmax (fp64 sum) without the clamp
        float mx = NEG;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = fmaxf(mx, a[j][e]);
        mx = wave_max(mx);
        double se = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) se += (double)exp_term(a[j][e] - mx);
        se = wave_sum(se);
        const double lse = (double)mx + log(se);
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) a[j][e] = (float)((double)a[j][e] - lse);
    }
    int x0rec = 0;
    if (LOSS) {     // arg-max of log_x0_recon = clamp(log_softmax) over k < K, row K = -70 competing (first maximum wins)
        float best0 = NEG; int best0_k = 0;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * lane + 256 * j + e;
                if (FULL || k < K) {
                    const float xr = clamp70(a[j][e]);
                    if (xr > best0) { best0 = xr; best0_k = k; }
                }
            }
        if (lane == 0 && -70.f > best0) { best0 = -70.f; best0_k = K; }
        x0rec = wave_argmax(best0, best0_k);
    }
    const int64_t t = d.t_dev[b];
    const StepSched s = load_sched(sp.p, t, d.T);
    const int xt = (int)d.xt[pos], x0 = (int)d.x0[pos];
    const bool masked = (xt == K);
    const float qt_hit = lae(0.f + s.lca, s.lcb), qt_miss = lae(LOG_ZERO + s.lca, s.lcb);
    const float q1_hit = lae(0.f + s.la, s.lb), q1_miss = lae(LOG_ZERO + s.la, s.lb);
    // Everything that depends only on the position is wave-uniform (pos comes through readfirstlane, so x_t, x_0, t and the schedule
    // row are scalar loads).  The two classes that are special -- k = x_t (the "hit" transition constants) and k = x_0 (the one-hot of
    // the true posterior) -- sit in register quads xj = x_t / 256 and x0j = x_0 / 256: every other quad runs with scalar constants, and
    // only those (at most two) quads evaluate per-class selects.  With a select per class in every pass the compiler kept 64-entry
    // vectors of them alive across the passes: 256 VGPRs + AGPR / scratch spills and one wave per SIMD.
    // (named scalars, not the struct: a struct captured by reference in the class-walking lambdas is demoted to scratch memory)
    const float s_pca = s.pca, s_pcb = s.pcb, s_p1mcc = s.p1mcc, s_pcc = s.pcc, s_lcc = s.lcc, s_lc = s.lc;
    const int xj = masked ? -1 : (xt >> 8), x0j = x0 >> 8;
    const float qt_c = masked ? s_lcc : qt_miss, q1_c = masked ? s_lc : q1_miss;       // the constants of a plain class
    const float E30 = expf(LOG_ZERO);
    // per-sample weights
    const float m0 = (t == 0) ? 1.f : 0.f;
    const float mw = masked ? d.mw_mask : d.mw_other;
    const float inv = 1.f / (d.pt[b] * (float)d.B * (float)d.L);
    const float w = d.adaptive ? ((1.f - (float)t / (float)d.T) + 1.0f) : 1.0f;
    const float g_kl = (1.f - m0) * mw * inv;
    const float g_nll = m0 * (1.f + w * d.aux_weight) * inv;
    const float g_aux = (1.f - m0) * w * d.aux_weight * mw * inv;
    // walks the classes of the row: f(j, e, k, log_qt, log_q1, lx0, w0) with the constants of class k
    auto for_classes = [&](auto f) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            if (j == xj || j == x0j) {                                                  // scalar branch
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 4 * lane + 256 * j + e;
                    if (FULL || k < K) {
                        const bool hit = !masked && k == xt, tru = k == x0;
                        f(j, e, k, hit ? qt_hit : qt_c, hit ? q1_hit : q1_c, tru ? 0.f : LOG_ZERO, tru ? 1.f : E30);
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 4 * lane + 256 * j + e;
                    if (FULL || k < K) f(j, e, k, qt_c, q1_c, LOG_ZERO, E30);
                }
            }
        }
    };
    // normalisers of the model / true posteriors
    float mxm = LOG_ZERO, mxt = LOG_ZERO;
    for_classes([&](int j, int e, int, float log_qt, float, float lx0, float) {
        mxm = fmaxf(mxm, clamp70(a[j][e]) - log_qt);
        mxt = fmaxf(mxt, lx0 - log_qt);
    });
    mxm = wave_max(mxm); mxt = wave_max(mxt);
    float sem = 0.f, set = 0.f;
    for_classes([&](int j, int e, int, float log_qt, float, float lx0, float) {
        sem += exp_term((clamp70(a[j][e]) - log_qt) - mxm);
        set += exp_term((lx0 - log_qt) - mxt);
    });
    sem = wave_sum(sem) + expf(LOG_ZERO - mxm);
    set = wave_sum(set) + expf(LOG_ZERO - mxt);
    const float Sm = mxm + logf(sem), St = mxt + logf(set);
    // pass A: Gqn_c and the gradient reaching S.  The per-class gradient under construction lives in LDS (one 16-byte slot per lane
    // and register quad, lane-contiguous: conflict-free b128 accesses), not in a second 64-register array.
    extern __shared__ __attribute__((aligned(16))) float gq_lds[];
    float* const gqs = gq_lds + (((threadIdx.x >> 6) * J) * 64 + lane) * 4;            // class (j, e) at gqs[256 j + e]
    float sumGe = 0.f, sumGqn = 0.f;
    float kl = 0.f, nll = 0.f, aux = 0.f;           // LOSS: the forward kernel's three sums and the arg-max of log_model
    float bestm = NEG; int bestm_k = 0;
    for_classes([&](int j, int e, int k, float log_qt, float log_q1, float lx0, float w0) {
        const float xr = clamp70(a[j][e]);
        const float qn = (xr - log_qt) - Sm;
        const float ee = lae(qn + s_pca, s_pcb);
        const float pre = ee + log_q1 + Sm;
        const float ltr = clamp70(lae(((lx0 - log_qt) - St) + s_pca, s_pcb) + log_q1 + St);
        const float eltr = exp_le0(ltr);
        const float G = -(g_kl * eltr + g_nll * w0);
        const float Ge = (pre >= -70.f && pre <= 0.f) ? G : 0.f;
        const float Gqn = Ge * exp_le0((qn + s_pca) - ee);
        gqs[256 * j + e] = Gqn;
        sumGe += Ge; sumGqn += Gqn;
        if (LOSS) {
            const float lm = clamp70(pre);
            kl += eltr * (ltr - lm);
            nll += w0 * lm;
            aux += w0 * (lx0 - xr);
            if (lm > bestm) { bestm = lm; bestm_k = k; }
        }
    });
    sumGe = wave_sum(sumGe); sumGqn = wave_sum(sumGqn);
    if (LOSS) { kl = wave_sum(kl); nll = wave_sum(nll); aux = wave_sum(aux); }
    {   // the [MASK] class: q_K is a constant, it only feeds S
        const float log_q1K = masked ? 0.f : LOG_ZERO;
        const float qnK = LOG_ZERO - Sm;
        const float eK = lae(qnK + s_p1mcc, s_pcc);
        const float preK = eK + log_q1K + Sm;
        const float ltK = clamp70(lae((LOG_ZERO - St) + s_p1mcc, s_pcc) + log_q1K + St);
        const float eltK = expf(ltK);
        const float GK = -(g_kl * eltK + g_nll * (x0 == K ? 1.f : E30));
        const float GeK = (preK >= -70.f && preK <= 0.f) ? GK : 0.f;
        sumGe += GeK;
        sumGqn += GeK * expf((qnK + s_p1mcc) - eK);
        if (LOSS) {
            const float lmK = clamp70(preK);
            kl += eltK * (ltK - lmK);
            nll += (x0 == K ? 1.f : E30) * lmK;
            if (lane == 0 && lmK > bestm) { bestm = lmK; bestm_k = K; }
        }
    }
    if (LOSS) {
        const int xt1 = wave_argmax(bestm, bestm_k);
        if (lane == 0) {
            d.kl[pos] = kl * mw;
            d.nll[pos] = -nll;
            d.aux[pos] = aux * mw;
            d.x0_recon[pos] = x0rec;
            d.xt1_recon[pos] = xt1;
        }
    }
    const float GS = sumGe - sumGqn;
    // pass B: through q -> r -> clamp -> log_softmax
    float sumGa = 0.f;
    for_classes([&](int j, int e, int, float log_qt, float, float, float w0) {
        const float r = clamp70(a[j][e]);
        const float pi = exp_le0((r - log_qt) - Sm);
        float Gr = gqs[256 * j + e] + GS * pi;
        Gr -= g_aux * w0;
        const float Ga = (a[j][e] >= -70.f && a[j][e] <= 0.f) ? Gr : 0.f;
        gqs[256 * j + e] = Ga;
        sumGa += Ga;
    });
    sumGa = wave_sum(sumGa);
    float* drow = d.dlogits + pos * (int64_t)K;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = 4 * lane + 256 * j;
        if (FULL || k < K) {
            float4 o;
            const float4 gv = *reinterpret_cast<const float4*>(gqs + 256 * j);
            // softmax probabilities of the gradient (relative error of exp_term: |a| 1.7e-7, at most 1.2e-5 and only where p < e^-69)
            o.x = gv.x - exp_term(a[j][0]) * sumGa; o.y = gv.y - exp_term(a[j][1]) * sumGa;
            o.z = gv.z - exp_term(a[j][2]) * sumGa; o.w = gv.w - exp_term(a[j][3]) * sumGa;
            *reinterpret_cast<float4*>(drow + k) = o;
        }
    }
}

}  // namespace gsdd

using namespace gsdd;

// false if one of the eight schedule buffers is null
static bool fill_sched(SchedPtrs& sp, const float* const* sched) {
    for (int i = 0; i < 8; ++i) {
        if (sched[i] == nullptr) return false;
        sp.p[i] = sched[i];
    }
    return true;
}

// the per-sample reductions and the scalar loss from what the loss (or the fused loss + gradient) kernel left in d's outputs
static void launch_train_finalize(const gsdd_train_desc* d, hipStream_t st) {
    TrainFinArgs f;
    f.kl = d->kl; f.nll = d->nll; f.aux = d->aux; f.x0 = d->x0; f.xt = d->xt; f.x0_recon = d->x0_recon;
    f.xt1_recon = d->xt1_recon; f.t_dev = d->t_dev; f.pt = d->pt; f.B = d->B; f.L = d->L; f.T = d->T;
    f.aux_weight = d->aux_weight; f.adaptive = d->adaptive_aux; f.Lt_history = d->Lt_history; f.Lt_count = d->Lt_count;
    f.loss = d->loss; f.per_sample = d->per_sample;
    hipLaunchKernelGGL(d3pm_train_finalize_kernel, dim3(1), dim3(256), 0, st, f);
}

extern "C" int gsdd_d3pm_step(const gsdd_step_desc* d, void* stream) {
    GSDD_CHECK_ARG(d != nullptr, "null descriptor");
    GSDD_CHECK_ARG(d->logits_c && d->tok_in && d->tok_out && d->t_dev && d->stream_dev, "null pointer");
    GSDD_CHECK_ARG(d->B > 0 && d->L > 0 && d->T > 0, "bad sizes");
    GSDD_CHECK_ARG(d->K >= 4 && d->K % 4 == 0 && d->K <= 8192, "K must be a multiple of 4 in [4, 8192]");
    SchedPtrs sp;
    GSDD_CHECK_ARG(fill_sched(sp, d->sched), "null schedule buffer");
    const int64_t npos = (int64_t)d->B * d->L;
    const dim3 grid((unsigned)((npos + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const bool dbg = d->post_dbg != nullptr || d->x0_dbg != nullptr;
    const bool trunc = d->trunc_rate != 0.f;
    GSDD_CHECK_ARG(d->occupancy == 0 || d->occupancy == 2 || d->occupancy == 3, "occupancy: 0 (auto), 2 or 3 waves per SIMD");
    GSDD_CHECK_ARG(d->post_skip >= 0, "post_skip must be >= 0");
    GSDD_CHECK_ARG(d->trunc_rate == 0.f || (d->trunc_rate > 0.f && d->trunc_rate < 1.f), "trunc_rate must be 0 (off) or in (0, 1)");
    if (d->known != nullptr) {                     // positions with a given clean token: the d3pm_step_known*_kernel families
        GSDD_CHECK_ARG(d->x_known != nullptr, "known needs x_known");
        GSDD_CHECK_ARG(d->known_mode == 0 || d->known_mode == 1, "known_mode: 0 (renoise) or 1 (hold)");
        GSDD_CHECK_ARG(!dbg, "known cannot be combined with post_dbg / x0_dbg");
        // FULL at K = 4096 only
        if (d->K == 4096 && !trunc) hipLaunchKernelGGL((d3pm_step_known_kernel<16, true>), grid, block, 0, st, *d, sp);
        else if (d->K == 4096) hipLaunchKernelGGL((d3pm_step_known_trunc_kernel<16, true>), grid, block, 0, st, *d, sp);
        else for_class_width(d->K, [&](auto jc) {
            constexpr int J = decltype(jc)::value;
            if (!trunc) hipLaunchKernelGGL((d3pm_step_known_kernel<J, false>), grid, block, 0, st, *d, sp);
            else hipLaunchKernelGGL((d3pm_step_known_trunc_kernel<J, false>), grid, block, 0, st, *d, sp);
        });
    } else if (trunc) {                            // top-r truncated sampling: the d3pm_step_trunc_kernel family, FULL at K = 4096 only
        if (d->K == 4096 && !dbg) hipLaunchKernelGGL((d3pm_step_trunc_kernel<16, true, false>), grid, block, 0, st, *d, sp);
        else if (d->K == 4096) hipLaunchKernelGGL((d3pm_step_trunc_kernel<16, true, true>), grid, block, 0, st, *d, sp);
        else for_class_width(d->K, [&](auto jc) {
            constexpr int J = decltype(jc)::value;
            if (!dbg) hipLaunchKernelGGL((d3pm_step_trunc_kernel<J, false, false>), grid, block, 0, st, *d, sp);
            else hipLaunchKernelGGL((d3pm_step_trunc_kernel<J, false, true>), grid, block, 0, st, *d, sp);
        });
    } else if (d->K == 4096 && !dbg && d->occupancy != 3) {    // the production shape: OCC = 2, no scratch (see the kernel's note)
        hipLaunchKernelGGL((d3pm_step_kernel<16, true, false, 2>), grid, block, 0, st, *d, sp);
    } else {                                       // the plain family: FULL at every K == 256 J, OCC = 3
        for_class_width(d->K, [&](auto jc) {
            constexpr int J = decltype(jc)::value;
            const bool full = d->K == 256 * J;
            if (full && !dbg) hipLaunchKernelGGL((d3pm_step_kernel<J, true, false>), grid, block, 0, st, *d, sp);
            else if (full) hipLaunchKernelGGL((d3pm_step_kernel<J, true, true>), grid, block, 0, st, *d, sp);
            else if (!dbg) hipLaunchKernelGGL((d3pm_step_kernel<J, false, false>), grid, block, 0, st, *d, sp);
            else hipLaunchKernelGGL((d3pm_step_kernel<J, false, true>), grid, block, 0, st, *d, sp);
        });
    }
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_d3pm_q_sample(const int64_t* x0, int64_t* xt, int B, int L, int K, int T,
                                  const float* const* sched, const int64_t* t_dev, uint64_t seed,
                                  const int64_t* stream_dev, int64_t row0, void* stream) {
    GSDD_CHECK_ARG(x0 && xt && sched && t_dev && stream_dev, "null pointer");
    GSDD_CHECK_ARG(B > 0 && L > 0 && T > 0 && K >= 4 && K % 4 == 0, "bad sizes");
    SchedPtrs sp;
    GSDD_CHECK_ARG(fill_sched(sp, sched), "null schedule buffer");
    const int64_t npos = (int64_t)B * L;
    hipLaunchKernelGGL(d3pm_q_sample_kernel, dim3((unsigned)((npos + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x0,
                       xt, B, L, K, T, sp, t_dev, seed, stream_dev, row0);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_advance(int64_t* t_dev, int B, int64_t dt, int64_t* stream_dev, int64_t ds, void* stream) {
    GSDD_CHECK_ARG(B >= 0 && B <= 65536, "bad B");
    const int n = B > 0 ? B : 1;
    hipLaunchKernelGGL(advance_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, t_dev, B, dt,
                       stream_dev, ds);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_advance_floor(int64_t* t_dev, int B, int64_t dt, int64_t t_min, int64_t* stream_dev, int64_t ds,
                                  void* stream) {
    GSDD_CHECK_ARG(B >= 0 && B <= 65536, "bad B");
    const int n = B > 0 ? B : 1;
    hipLaunchKernelGGL(advance_floor_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, t_dev, B, dt, t_min,
                       stream_dev, ds);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_philox_uniform(uint64_t seed, int64_t stream_id, int64_t row0, int64_t n_rows, int n_cols,
                                   float* out, void* stream) {
    GSDD_CHECK_ARG(out != nullptr && n_rows > 0 && n_cols > 0, "bad args");
    const int64_t n = n_rows * (int64_t)((n_cols + 3) / 4);
    hipLaunchKernelGGL(philox_uniform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       seed, (uint32_t)stream_id, row0, n_rows, n_cols, out);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_d3pm_train_loss(const gsdd_train_desc* d, void* stream) {
    GSDD_CHECK_ARG(d != nullptr, "null descriptor");
    GSDD_CHECK_ARG(d->logits && d->x0 && d->xt && d->t_dev && d->pt && d->kl && d->nll && d->aux && d->x0_recon &&
                   d->xt1_recon && d->Lt_history && d->Lt_count && d->loss && d->per_sample, "null pointer");
    GSDD_CHECK_ARG(d->B > 0 && d->B <= 1024 && d->L > 0 && d->T > 0, "bad sizes (B <= 1024)");
    GSDD_CHECK_ARG(d->K >= 4 && d->K % 4 == 0 && d->K <= 8192, "K must be a multiple of 4 in [4, 8192]");
    SchedPtrs sp;
    GSDD_CHECK_ARG(fill_sched(sp, d->sched), "null schedule buffer");
    TrainArgs a;
    a.logits = d->logits; a.x0 = d->x0; a.xt = d->xt; a.t_dev = d->t_dev; a.B = d->B; a.L = d->L; a.K = d->K; a.T = d->T;
    a.mw_mask = d->mask_weight[0]; a.mw_other = d->mask_weight[1];
    a.kl = d->kl; a.nll = d->nll; a.aux = d->aux; a.x0_recon = d->x0_recon; a.xt1_recon = d->xt1_recon; a.probs = d->probs;
    const int64_t npos = (int64_t)d->B * d->L;
    const dim3 grid((unsigned)((npos + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (d->K == 4096) hipLaunchKernelGGL((d3pm_train_loss_kernel<16, true>), grid, block, 0, st, a, sp);      // FULL at K = 4096 only
    else for_class_width(d->K, [&](auto jc) {
        hipLaunchKernelGGL(d3pm_train_loss_kernel<decltype(jc)::value>, grid, block, 0, st, a, sp);
    });
    GSDD_CHECK_LAUNCH();
    launch_train_finalize(d, st);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

static int train_bwd_launch(const gsdd_train_desc* d, float* dlogits, bool with_loss, void* stream);

extern "C" int gsdd_d3pm_train_loss_bwd(const gsdd_train_desc* d, float* dlogits, void* stream) {
    return train_bwd_launch(d, dlogits, false, stream);
}

extern "C" int gsdd_d3pm_train_loss_grad(const gsdd_train_desc* d, float* dlogits, void* stream) {
    GSDD_CHECK_ARG(d != nullptr && dlogits != nullptr, "null pointer");
    GSDD_CHECK_ARG(d->kl && d->nll && d->aux && d->x0_recon && d->xt1_recon && d->Lt_history && d->Lt_count && d->loss && d->per_sample,
                   "null pointer");
    GSDD_CHECK_ARG(d->probs == nullptr, "the fused pass does not write probs: call gsdd_d3pm_train_loss + gsdd_d3pm_train_loss_bwd");
    GSDD_CHECK_ARG(d->B <= 1024, "bad sizes (B <= 1024)");
    const int rc = train_bwd_launch(d, dlogits, true, stream);
    if (rc != GSDD_OK) return rc;
    launch_train_finalize(d, (hipStream_t)stream);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

static int train_bwd_launch(const gsdd_train_desc* d, float* dlogits, bool with_loss, void* stream) {
    GSDD_CHECK_ARG(d != nullptr && dlogits != nullptr, "null pointer");
    GSDD_CHECK_ARG(d->logits && d->x0 && d->xt && d->t_dev && d->pt, "null pointer");
    GSDD_CHECK_ARG(d->B > 0 && d->L > 0 && d->T > 0 && d->K >= 4 && d->K % 4 == 0 && d->K <= 8192, "bad sizes");
    SchedPtrs sp;
    GSDD_CHECK_ARG(fill_sched(sp, d->sched), "null schedule buffer");
    TrainBwdArgs a;
    a.logits = d->logits; a.x0 = d->x0; a.xt = d->xt; a.t_dev = d->t_dev; a.pt = d->pt;
    a.B = d->B; a.L = d->L; a.K = d->K; a.T = d->T;
    a.mw_mask = d->mask_weight[0]; a.mw_other = d->mask_weight[1]; a.aux_weight = d->aux_weight; a.adaptive = d->adaptive_aux;
    a.dlogits = dlogits;
    a.kl = d->kl; a.nll = d->nll; a.aux = d->aux; a.x0_recon = d->x0_recon; a.xt1_recon = d->xt1_recon;
    const int64_t npos = (int64_t)d->B * d->L;
    const dim3 grid((unsigned)((npos + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    // dynamic LDS: one float4 per (wave, register quad, lane) = 4 KB * J per workgroup (64 KB at K = 4096: two workgroups per CU)
    if (d->K > 4096) {                             // J = 32 (4096 < K <= 8192) needs 128 KB of dynamic LDS: above the 64 KB default
        int dev = 0, lds_max = 0;
        GSDD_CHECK_HIP(hipGetDevice(&dev));
        GSDD_CHECK_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
        GSDD_CHECK_ARG(lds_max >= 4096 * 32, "K > 4096 needs 128 KB of LDS per workgroup (gfx950 has 160 KB)");
        GSDD_ONCE_PER_DEVICE(attr_done,
            GSDD_CHECK_HIP(hipFuncSetAttribute((const void*)d3pm_train_bwd_kernel<32, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 4096 * 32));
            GSDD_CHECK_HIP(hipFuncSetAttribute((const void*)d3pm_train_bwd_kernel<32, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 4096 * 32));
        );
    }
    // FULL at K = 4096, the workload's class count, only: every register slot holds a class
    if (d->K == 4096 && with_loss) hipLaunchKernelGGL((d3pm_train_bwd_kernel<16, true, true>), grid, block, (size_t)4096 * 16, st, a, sp);
    else if (d->K == 4096) hipLaunchKernelGGL((d3pm_train_bwd_kernel<16, false, true>), grid, block, (size_t)4096 * 16, st, a, sp);
    else for_class_width(d->K, [&](auto jc) {
        constexpr int J = decltype(jc)::value;
        if (with_loss) hipLaunchKernelGGL((d3pm_train_bwd_kernel<J, true>), grid, block, (size_t)4096 * J, st, a, sp);
        else hipLaunchKernelGGL((d3pm_train_bwd_kernel<J, false>), grid, block, (size_t)4096 * J, st, a, sp);
    });
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}
