// Long clips: the two device ops of the sliding-window rollout (d3pm.long_plan, DiffusionTransformer.sample_long, VQVAE.decode_long).
//
// A long token grid of n latent frames is sampled as W windows of F frames that overlap by k: window w covers long frames
// [w s, w s + F), s = F - k, and is conditioned on the last k frames of window w - 1 (known-token conditioned sampling).  Long frame
// f takes its tokens from the first window that sampled it: window 0 for f < F, window w >= 1 for f in [w s + k, w s + F).
//
// d3pm_window_slide_kernel -- the op between two windows, one launch per lane, on the lane's own fixed buffers, so that the graphs
// captured for the step / jump kinds replay unchanged in every window.  Per token of the finished window (Bs clips of F hw tokens):
//   * a frame the window contributes goes to the lane's rows of the long buffer (B, n hw); frames >= n are dropped (the last window),
//   * the last k frames become x_known[:, :k hw], the clean tokens of the next window; a token outside [0, K) there is counted
//     ([MASK] = K is no clean token: the host reads the counter once per call),
//   * known <- 1 on the first k hw positions, 0 behind them; tok <- [MASK]; t2 <- t0 on its n_t2 rows.
// The finished window's index is device state, read by every workgroup at its start: state[0] = the index, state[1] = workgroups
// that have finished.  The last workgroup to finish moves state[0] on and clears state[1] (a device-scope counter behind a fence:
// every workgroup has read state[0] before it arrives), so a captured launch serves every window and nothing else has to run between
// two windows.  An index outside [0, n] (never produced by the rollout) writes nothing to the long buffer.
// final != 0 is the launch behind the last window: only the copy to the long buffer, no state moves.
// Every fill is a store of this kernel (no hipMemsetAsync inside what a graph records); no LDS, no scratch.  At 32 KB of tokens per
// clip the launch is latency-bound: one token per thread.
//
// clip_window_blend_kernel -- merges one decoded window (BC planes of Fw frames of HW floats) into the long clip (BC planes of Fo
// frames) at output frame f0.  A plane's frames are contiguous in both, so each plane is one run of min(Fw, Fo - f0) HW floats:
// elements [0, ov) (the n_ov overlapped frames, decoded by the window before as well) are crossfaded in fp32,
// out <- out + a_j (win - out), a_j = (j + 1) / (n_ov + 1) for frame j of the overlap; elements behind them are copied; elements in
// front of `begin` are not touched ("keep": begin = ov; "replace" is the copy with no overlap).  Nothing behind frame Fo is written.
// 16-byte accesses where the run starts on a 16-byte boundary in both buffers, for the vectors that lie wholly on one side of ov;
// the vector that straddles it, the run's last H W Fw mod 4 floats and unaligned runs go element by element.
#include "common.hpp"

namespace gsdd {

__global__ __launch_bounds__(256) void d3pm_window_slide_kernel(int64_t* __restrict__ tok, int64_t* __restrict__ long_tok,
                                                                int64_t* __restrict__ x_known, uint8_t* __restrict__ known,
                                                                int64_t* __restrict__ t2, int64_t* state, int* __restrict__ bad,
                                                                int Bs, int F, int hw, int k, int n, int K, int64_t t0, int n_t2,
                                                                int final_copy) {
    const int64_t w = __atomic_load_n(&state[0], __ATOMIC_RELAXED);          // the finished window
    const int s = F - k;
    const int64_t Lw = (int64_t)F * hw, total = (int64_t)Bs * Lw, row = (int64_t)n * hw;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < total) {
        const int64_t b = e / Lw, p = e - b * Lw;
        const int fr = (int)(p / hw);
        const int64_t v = tok[e];
        if (w >= 0 && w <= (int64_t)n && fr >= (w == 0 ? 0 : k)) {
            const int64_t lf = w * s + fr;                                    // (<= n F + F: no overflow)
            if (lf < (int64_t)n) long_tok[b * row + lf * hw + (p - (int64_t)fr * hw)] = v;
        }
        if (!final_copy) {
            if (fr >= s) {
                x_known[e - (int64_t)s * hw] = v;
                if (v < 0 || v >= (int64_t)K) atomicAdd(bad, 1);
            }
            known[e] = fr < k ? 1 : 0;
            tok[e] = K;
            if (e < (int64_t)n_t2) t2[e] = t0;
        }
    }
    if (final_copy) return;
    __syncthreads();                                                          // every thread of the workgroup has read state[0]
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned long long arrived = atomicAdd(reinterpret_cast<unsigned long long*>(&state[1]), 1ull);
        if (arrived == (unsigned long long)gridDim.x - 1ull) {               // the last workgroup: nobody reads state[0] any more
            __atomic_store_n(&state[1], (int64_t)0, __ATOMIC_RELAXED);
            __atomic_store_n(&state[0], w + 1, __ATOMIC_RELAXED);
        }
    }
}

template <bool LINEAR>
__device__ __forceinline__ void blend_one(const float* __restrict__ src, float* __restrict__ dst, int64_t e, int64_t begin, int64_t ov,
                                          int HW, float denom) {
    if (e < begin) return;
    const float wv = src[e];
    if (LINEAR && e < ov) {
        const float o = dst[e], a = (float)(e / HW + 1) / denom;
        dst[e] = o + a * (wv - o);
    } else {
        dst[e] = wv;
    }
}

template <bool LINEAR>
__global__ __launch_bounds__(256) void clip_window_blend_kernel(const float* __restrict__ win, float* __restrict__ out, int Fw, int HW,
                                                                int Fo, int f0, int n_ov, int64_t begin) {
    const int64_t plane = blockIdx.y;
    const int frames = min(Fw, Fo - f0);
    const int64_t len = (int64_t)frames * HW, ov = LINEAR ? (int64_t)n_ov * HW : 0;
    const float* src = win + plane * Fw * HW;
    float* dst = out + (plane * Fo + f0) * HW;
    const float denom = (float)(n_ov + 1);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
    const int64_t nvec = vec ? len / 4 : 0;
    for (int64_t v = tid; v < nvec; v += stride) {
        const int64_t e = 4 * v;
        if (e >= begin && e >= ov) {                                          // copied
            reinterpret_cast<float4*>(dst)[v] = reinterpret_cast<const float4*>(src)[v];
        } else if (LINEAR && e >= begin && e + 3 < ov) {                      // crossfaded, possibly across a frame seam
            const float4 wv = reinterpret_cast<const float4*>(src)[v];
            float4 o = reinterpret_cast<float4*>(dst)[v];
            o.x = o.x + ((float)(e / HW + 1) / denom) * (wv.x - o.x);
            o.y = o.y + ((float)((e + 1) / HW + 1) / denom) * (wv.y - o.y);
            o.z = o.z + ((float)((e + 2) / HW + 1) / denom) * (wv.z - o.z);
            o.w = o.w + ((float)((e + 3) / HW + 1) / denom) * (wv.w - o.w);
            reinterpret_cast<float4*>(dst)[v] = o;
        } else {                                                              // straddles `begin` or the end of the overlap
#pragma unroll
            for (int i = 0; i < 4; ++i) blend_one<LINEAR>(src, dst, e + i, begin, ov, HW, denom);
        }
    }
    for (int64_t e = 4 * nvec + tid; e < len; e += stride) blend_one<LINEAR>(src, dst, e, begin, ov, HW, denom);
}

}  // namespace gsdd

using namespace gsdd;

extern "C" int gsdd_d3pm_window_slide(int64_t* tok, int64_t* long_tok, int64_t* x_known, uint8_t* known, int64_t* t2, int64_t* state,
                                      int* bad, int Bs, int F, int hw, int k, int n, int K, int64_t t0, int n_t2, int final_copy,
                                      void* stream) {
    GSDD_CHECK_ARG(tok && long_tok && state, "null pointer");
    GSDD_CHECK_ARG(final_copy == 0 || final_copy == 1, "final_copy must be 0 or 1");
    GSDD_CHECK_ARG(final_copy || (x_known && known && t2 && bad), "null pointer");
    GSDD_CHECK_ARG(Bs > 0 && F > 0 && hw > 0 && n > 0, "bad sizes");
    GSDD_CHECK_ARG(k >= 1 && k <= F - 1, "the overlap k must lie in [1, F - 1]");
    GSDD_CHECK_ARG(n >= F, "n (long frames) must be at least F (the window's frames)");
    GSDD_CHECK_ARG(K >= 1 && t0 >= 0, "K must be >= 1 and t0 >= 0");
    GSDD_CHECK_ARG(n_t2 >= 0 && (int64_t)n_t2 <= (int64_t)Bs * F * hw, "n_t2 must lie in [0, Bs F hw]");
    const int64_t total = (int64_t)Bs * F * hw;
    GSDD_CHECK_ARG(total < ((int64_t)1 << 31) && (int64_t)n * hw < ((int64_t)1 << 40), "window or long row too large");
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    hipLaunchKernelGGL(d3pm_window_slide_kernel, grid, block, 0, (hipStream_t)stream, tok, long_tok, x_known, known, t2, state, bad,
                       Bs, F, hw, k, n, K, t0, n_t2, final_copy);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_clip_window_blend(const float* win, float* out, int BC, int Fw, int HW, int Fo, int f0, int n_ov, int mode,
                                      void* stream) {
    GSDD_CHECK_ARG(win && out, "null pointer");
    GSDD_CHECK_ARG(BC > 0 && BC <= 65535 && Fw > 0 && HW > 0 && Fo > 0, "bad sizes");
    GSDD_CHECK_ARG(Fo >= Fw, "the long clip must hold at least one window (n >= F)");
    GSDD_CHECK_ARG(n_ov >= 0 && n_ov < Fw, "the overlap must be shorter than the window (k < F)");
    GSDD_CHECK_ARG(f0 >= 0 && f0 < Fo, "the window must start inside the long clip");
    GSDD_CHECK_ARG(n_ov == 0 || f0 > 0, "an overlapped window cannot be the first");
    GSDD_CHECK_ARG(mode >= GSDD_BLEND_LINEAR && mode <= GSDD_BLEND_REPLACE, "mode must be GSDD_BLEND_LINEAR, _KEEP or _REPLACE");
    GSDD_CHECK_ARG((int64_t)Fw * HW < ((int64_t)1 << 31) && (int64_t)BC * Fo * HW < ((int64_t)1 << 40), "clip too large");
    GSDD_CHECK_ARG((reinterpret_cast<uintptr_t>(win) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0, "float operands off 4-byte alignment");
    const int frames = Fw < Fo - f0 ? Fw : Fo - f0;
    const int64_t len = (int64_t)frames * HW, begin = mode == GSDD_BLEND_KEEP ? (int64_t)n_ov * HW : 0;
    if (begin >= len) return GSDD_OK;                                         // "keep" of a window that adds no frame: nothing to write
    const int64_t per_block = 256 * 4 * 4;                                    // four vectors per thread
    const dim3 grid((unsigned)((len + per_block - 1) / per_block), (unsigned)BC), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (mode == GSDD_BLEND_LINEAR && n_ov > 0)
        hipLaunchKernelGGL(clip_window_blend_kernel<true>, grid, block, 0, st, win, out, Fw, HW, Fo, f0, n_ov, begin);
    else
        hipLaunchKernelGGL(clip_window_blend_kernel<false>, grid, block, 0, st, win, out, Fw, HW, Fo, f0, n_ov, begin);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}
