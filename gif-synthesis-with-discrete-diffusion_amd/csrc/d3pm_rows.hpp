// Register-resident class rows of the D3PM kernels (d3pm_step.hip, d3pm_purity.hip): one wave64 owns one token position, lane owns
// quads k = 4*lane + 256*j; the restricted-range expf / logf, the reference's log_add_exp, the fp64-sum log_softmax, the wave
// log-sum-exp, the top-r truncation, the Gumbel transform and the first-index arg-max they share.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace gsdd {

constexpr float LOG_ZERO = -69.07755278982137f;  // log(1e-30)

// expf / logf restricted to the argument ranges this file feeds them.  Both run the device library's own
// arithmetic (two-constant log2(e) / ln 2 products around v_exp_f32 / v_log_f32, same constants, same order), so
// results are bit-identical to expf / logf on those ranges; what is dropped is the library's range plumbing
// (two compare+select pairs per expf, denormal pre-scaling and the inf/nan select per logf), which costs more issue
// slots than the arithmetic itself (tools/rate_probe6.hip: compares and selects issue at half the f32 add/mul rate).
//   exp_le0(x): x <= 0 (or -inf).  The lower clamp stands in for the library's "x < -103.28 -> 0" select:
//               exp(-104) < 2^-150 rounds to 0 in v_ldexp_f32, and it keeps a -inf / absurdly negative
//               argument away from the hi/lo product.
//   log_norm(x): x finite and >= 2^-126 (here always >= 1e-30).
//               CLAMP = false where the argument is known to be finite and of moderate size (differences of clamped
//               log-probabilities and schedule constants): the clamp is one more half-rate instruction.
template <bool CLAMP = true>
__device__ __forceinline__ float exp_le0(float x) {
    const float L2E_HI = __builtin_bit_cast(float, 0x3fb8aa3bu), L2E_LO = __builtin_bit_cast(float, 0x32a5705fu);
    if (CLAMP) x = fmaxf(x, -104.f);
    const float ph = x * L2E_HI;
    float pl = fmaf(x, L2E_HI, -ph);
    const float e = rintf(ph);
    pl = fmaf(x, L2E_LO, pl);
    const float a = (ph - e) + pl;
    return ldexpf(__builtin_amdgcn_exp2f(a), (int)e);
}
// exp(d), d <= 0 (or -inf), for the TERMS OF A SUM over classes: one product and v_exp_f32 (relative error ~ |d| * 1.7e-7, i.e. small
// exactly where the term is not).  A log-sum-exp enters every class of its row as the same additive constant, which the arg-max at
// the end of the step does not see; what its accuracy decides is how often x - lse rounds to the neighbouring float.  With these
// terms the fp64 sum over a row is accurate to ~1e-9 relative (the largest term is exp(0) = 1 exactly), the same as with the
// 12-instruction exp_le0, which is kept for the per-class values (log_add_exp), where every class has its own error.
#ifdef GSDD_DEV_EXACT_SUM_EXP      // development A/B only (tools/neartie_diff.py): the sum terms on the library-exact exponential, as before 2f17ed5
__device__ __forceinline__ float exp_term(float d) { return exp_le0(d); }
#else
__device__ __forceinline__ float exp_term(float d) { return __builtin_amdgcn_exp2f(d * 1.44269504088896340736f); }
#endif
__device__ __forceinline__ float log_norm(float x) {
    const float LN2_HI = __builtin_bit_cast(float, 0x3f317217u), LN2_LO = __builtin_bit_cast(float, 0x3377d1cfu);
    const float r = __builtin_amdgcn_logf(x);
    const float ph = r * LN2_HI;
    float pl = fmaf(r, LN2_HI, -ph);
    pl = fmaf(r, LN2_LO, pl);
    return ph + pl;
}

// reference log_add_exp (:32-34): m + log(exp(a - m) + exp(b - m)), m = max(a, b).  One of the two exponentials is
// exp(0) = 1 exactly and the other one's argument is -|a - b| exactly, so a single exp gives the same bits.
__device__ __forceinline__ float lae(float a, float b) {
    const float m = fmaxf(a, b);
    return m + log_norm(1.f + exp_le0(-fabsf(a - b)));   // clamped: a schedule constant may be log(0) = -inf (t - 1 wrap)
}
__device__ __forceinline__ float clamp70(float v) { return fminf(fmaxf(v, -70.f), 0.f); }

struct StepSched {
    float la, lb, lc, l1mc;          // per-step at t
    float lca, lcb, lcc, l1mcc;      // cumulative at t
    float pca, pcb, pcc, p1mcc;      // cumulative at t-1 (wrapped)
};

__device__ __forceinline__ StepSched load_sched(const float* const* s, int64_t t, int T) {
    StepSched r;
    r.la = s[0][t]; r.lb = s[1][t]; r.lc = s[2][t]; r.l1mc = s[3][t];
    r.lca = s[4][t]; r.lcb = s[5][t]; r.lcc = s[6][t]; r.l1mcc = s[7][t];
    const int64_t tp = (t - 1 + (T + 1)) % (T + 1);
    r.pca = s[4][tp]; r.pcb = s[5][tp]; r.pcc = s[6][tp]; r.p1mcc = s[7][tp];
    return r;
}

struct SchedPtrs { const float* p[8]; };

// log_softmax over the wave's row (fp64 sum/log), clamp to [-70,0]   (predict_start, :231-236)
// (d3pm_compose.hip's two-pass J = 32 path restates the two halves as row_lse / lsm_clamp, operation for operation: a change here goes there too)
template <int J>
__device__ __forceinline__ void log_softmax_clamp(float (&x)[J][4]) {
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
    const double lse = (double)mx + log(se);
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) x[j][e] = clamp70((float)((double)x[j][e] - lse));
}

// CLAMP = false: every slot holds a finite, bounded value (FULL rows of clamped log-probabilities)
template <int J, bool CLAMP = true>
__device__ __forceinline__ float wave_logsumexp(const float (&x)[J][4], float extra, bool has_extra) {
    float mx = has_extra ? extra : -INFINITY;
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) mx = fmaxf(mx, x[j][e]);
    mx = wave_max(mx);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) se += exp_term(x[j][e] - mx);
    se = wave_sum(se);
    if (has_extra) se += exp_le0(extra - mx);
    return mx + logf(se);
}

// order-preserving bits of a float: a < b  <=>  ordered(a) < ordered(b); every float (-inf included) maps above 0
__device__ __forceinline__ uint32_t ordered_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_float(uint32_t o) {       // the inverse
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// Top-r truncation of a final log p(x0 | x_t) row (VQ-Diffusion's predict_start_with_truncation, "top0.86r"): class k is kept iff
// the probability mass strictly above it, sum_{x_j > x_k} exp(x_j), is below rate; every other class drops to -70 (no renormalising:
// the posterior normalises itself).  Equal values are kept or cut together, the row maximum is always kept, and an entry already at
// -70 does not change either way.  No sort: the mass above a value v is non-increasing in v, so the cut value -- the smallest c with
// mass_above(c) < rate -- is found by bisection on the order-preserving integer image of the floats in [-70, 0] (at most 31 probes,
// each one compare-and-accumulate over the lane's slots on the exponentials kept in registers, plus one wave reduction).  The lane
// sums are fp32 in slot order, the sum across lanes is fp64: the 64 lane sums enter as the same binary tree whatever the lane.
// The probe loop's bounds and verdict are wave-uniform (scalar registers, scalar branch).  An empty slot (-inf, K < 256 J) stays -inf.
template <int J, bool FULL>
__device__ __forceinline__ void truncate_row(float (&x)[J][4], float rate, int lane, int K) {
    float p[J][4];
    float mx = -70.f;
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            p[j][e] = exp_le0(x[j][e]);                         // (an empty slot: exp(-inf) = 0)
            mx = fmaxf(mx, x[j][e]);
        }
    uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)ordered_bits(wave_max(mx)));   // mass_above(row maximum) = 0 < rate
    uint32_t lo = ordered_bits(-70.f) - 1u;                     // below every entry: "mass_above >= rate" by convention
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const float v = ordered_float(mid);
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) m += (x[j][e] > v) ? p[j][e] : 0.f;
        const bool below = (float)wave_sum((double)m) < rate;
        if (__builtin_amdgcn_readfirstlane((int)below)) hi = mid; else lo = mid;
    }
    const float cut = ordered_float(hi);
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const bool valid = FULL || (4 * lane + 256 * j) < K;
#pragma unroll
        for (int e = 0; e < 4; ++e) x[j][e] = valid ? ((x[j][e] >= cut) ? x[j][e] : -70.f) : -INFINITY;
    }
}

__device__ __forceinline__ float gumbel(float u) {  // log_sample_categorical (:355-356); u in [0, 1)
    return -log_norm(-log_norm(u + 1e-30f) + 1e-30f);
}

// arg-max of (val, idx) over the wave, first index wins ties (torch.argmax)
__device__ __forceinline__ int wave_argmax(float v, int idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(idx, o);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    return idx;
}

// The draw of a position whose clean token is given (gsdd_step_desc.known): Gumbel arg-max over the K + 1 classes of a forward
// marginal q(x_s | x_0 = tok), which has three values -- `hit` for class tok, `miss` for every other code, `mval` for [MASK] (q_pred of
// a log-one-hot row, as in d3pm_q_sample_kernel).  No row lives in registers: the wave walks the register slots of the posterior draw
// with that draw's Philox counters (quad k0 / 4 of global row `grow`, [MASK] = word 0 of quad K / 4 on lane (K / 4) % 64), so a
// position consumes the same uniforms whichever path it takes.  tok is wave-uniform: the hit is a scalar branch on j plus one lane
// compare.  Classes are visited in increasing k per lane and wave_argmax keeps the first index: torch.argmax's choice.
template <int J, bool FULL>
__device__ __forceinline__ int known_row_draw(int tok, float hit, float miss, float mval, int lane, int K, uint64_t seed,
                                              uint32_t stream_id, uint64_t grow) {
    const uint32_t kp4 = (uint32_t)((K + 1 + 3) / 4);
    const int xj = tok >> 8, xl = (tok >> 2) & 63, xe = tok & 3;
    const bool mine = (lane == xl);
    float best = -INFINITY;
    int best_k = 0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k0 = 4 * lane + 256 * j;
        if (FULL || k0 < K) {
            const float4 u4 = philox_uniform4(seed, stream_id, grow, kp4, (uint32_t)(k0 >> 2));
            const float u[4] = {u4.x, u4.y, u4.z, u4.w};
            if (j == xj) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = gumbel(u[e]) + ((mine && e == xe) ? hit : miss);
                    if (v > best) { best = v; best_k = k0 + e; }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = gumbel(u[e]) + miss;
                    if (v > best) { best = v; best_k = k0 + e; }
                }
            }
        }
    }
    if (lane == ((K >> 2) & 63)) {
        const float4 u4 = philox_uniform4(seed, stream_id, grow, kp4, (uint32_t)(K >> 2));
        const float v = gumbel(u4.x) + mval;
        if (v > best) { best = v; best_k = K; }
    }
    return wave_argmax(best, best_k);
}

// Host side: the one map from a class count K <= 8192 to the register quads per lane of the kernel that covers it.  Calls
// f(std::integral_constant<int, J>{}) with the smallest J in {1, 2, 4, 8, 16, 32} such that K <= 256 J; the caller's generic lambda
// picks the other template arguments of its kernel family (FULL, DBG, OCC, MODE) and launches.
template <class F>
void for_class_width(int K, F&& f) {
    if (K <= 256) f(std::integral_constant<int, 1>{});
    else if (K <= 512) f(std::integral_constant<int, 2>{});
    else if (K <= 1024) f(std::integral_constant<int, 4>{});
    else if (K <= 2048) f(std::integral_constant<int, 8>{});
    else if (K <= 4096) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 32>{});
}

}  // namespace gsdd
