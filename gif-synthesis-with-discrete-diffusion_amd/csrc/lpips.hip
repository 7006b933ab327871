// LPIPS (gsdd_amd/lpips.py; the rule in full: include/gsdd.h): the two ends of the metric that are its own.  What lies between them -- the
// AlexNet / VGG-16 convolutions and max pools -- is gsdd_gemm and gsdd_pool3d.
//
//   stem_rows        one thread per position of the first convolution's operand: frames [n][H][W + 2 padw] of 4 floats.  A pixel's three
//                    levels -- a float through gif_level, a byte as it is -- index the 3 x 256 table the caller formed on the host
//                    ((level / 127.5 - 1 - shift_c) / scale_c in fp64, rounded to fp32 once; staged in LDS), the fourth float and all four
//                    of a pad column are 0: the padding is zero in the SCALED space, which no level maps to.  One 16-byte store a thread.
//   layer_distance   rows [2n P][C] of one tap, pred frames first.  A row's C / 4 float4s are spread over G = min(64, 2^ceil(log2(C / 4)))
//                    lanes, so a wave holds 64 / G positions at a time: 4 at C = 64, where one position a wave would leave three quarters
//                    of it idle, and 1 at C = 512 with two float4s a lane.  Every element of both operands is read once and stays in
//                    registers: the two squared norms are xor butterflies over the G lanes, 1 / (sqrt(n) + 1e-10) is formed once per
//                    position and operand, and w (a ia - b ib)^2 is added, per lane and in fp64, over the positions the lane sees.  The
//                    same expressions in the same order serve a and b: equal halves give exactly 0.  A workgroup (4 waves) owns
//                    LD_ITERS * 4 * 64 / G consecutive positions of one frame pair; its lanes' sums meet in a fixed order (butterfly over
//                    the wave, the four waves in turn) and go to partials[pair][slot] as one double.  No atomics, nothing to zero, every
//                    word written by exactly one workgroup: safe to capture, the same bits in every run and whatever the batch holds.
#include "common.hpp"
#include "gif_device.hpp"

namespace gsdd {

constexpr int LP_THREADS = 256, LP_TABLE = 3 * 256, LP_MAX_PADW = 64;
constexpr int LD_THREADS = 256, LD_WAVES = LD_THREADS / WAVE, LD_ITERS = 8, LD_MAX_C = 512;
constexpr float LD_EPS = 1e-10f;

__global__ __launch_bounds__(LP_THREADS) void lpips_stem_rows_kernel(const void* __restrict__ x, int form, int T, int H, int W,
                                                                     int64_t frame0, int padw, int64_t total,
                                                                     const float* __restrict__ table, GifNorm nm,
                                                                     float4* __restrict__ out) {
    __shared__ float tab[LP_TABLE];
    for (int i = threadIdx.x; i < LP_TABLE; i += LP_THREADS) tab[i] = table[i];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= total) return;
    const int Wp = W + 2 * padw;
    const int64_t row = i / Wp;                                   // (frame of the chunk, y)
    const int xp = (int)(i - row * Wp), xx = xp - padw;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (xx >= 0 && xx < W) {
        const int64_t f = row / H;
        const int y = (int)(row - f * H);
        const int64_t frame = frame0 + f, b = frame / T, t = frame - b * T;
        const int64_t HW = (int64_t)H * W, pix = (int64_t)y * W + xx;
        int l0, l1, l2;
        if (form == 0) {
            const float* p = static_cast<const float*>(x) + (b * 3 * T + t) * HW + pix;
            const int64_t cs = (int64_t)T * HW;
            l0 = gif_level(p[0], nm.mean[0], nm.std[0]);
            l1 = gif_level(p[cs], nm.mean[1], nm.std[1]);
            l2 = gif_level(p[2 * cs], nm.mean[2], nm.std[2]);
        } else {
            const uint8_t* p = static_cast<const uint8_t*>(x) + (frame * HW + pix) * 3;
            l0 = p[0];
            l1 = p[1];
            l2 = p[2];
        }
        v = make_float4(tab[l0], tab[256 + l1], tab[512 + l2], 0.f);
    }
    out[i] = v;
}

// lanes a row of C / 4 float4s is spread over: the power of two at or above C / 4, 64 at the most
__host__ __device__ inline int ld_group(int C) {
    int g = 1;
    while (g < C / 4 && g < WAVE) g <<= 1;
    return g;
}
__host__ __device__ inline int64_t ld_rows_per_group(int C) { return (int64_t)LD_ITERS * LD_WAVES * (WAVE / ld_group(C)); }

__device__ __forceinline__ float ld_sq(const float4& v) { return (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }
__device__ __forceinline__ float ld_term(const float4& a, float ia, const float4& b, float ib, const float4& w) {
    const float dx = a.x * ia - b.x * ib, dy = a.y * ia - b.y * ib, dz = a.z * ia - b.z * ib, dw = a.w * ia - b.w * ib;
    return (w.x * (dx * dx) + w.y * (dy * dy)) + (w.z * (dz * dz) + w.w * (dw * dw));
}

__global__ __launch_bounds__(LD_THREADS) void lpips_layer_distance_kernel(const float4* __restrict__ feat, const float4* __restrict__ w,
                                                                          int64_t n, int64_t P, int C4, int G, int slots,
                                                                          double* __restrict__ partials) {
    __shared__ double wave_d[LD_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int R = WAVE / G, g = lane / G, q0 = lane - g * G, q1 = q0 + G;     // G = 64 alone has a second float4 (C4 <= 128)
    const int64_t pair = blockIdx.x / slots;
    const int slot = (int)(blockIdx.x - pair * slots);
    const bool has0 = q0 < C4, has1 = q1 < C4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 w0 = has0 ? w[q0] : zero, w1 = has1 ? w[q1] : zero;
    const float4* fa = feat + pair * P * C4;
    const float4* fb = feat + (n + pair) * P * C4;
    const int64_t p0 = (int64_t)slot * LD_ITERS * LD_WAVES * R + wave * R + g;

    double acc = 0.0;
#pragma unroll 2
    for (int it = 0; it < LD_ITERS; ++it) {
        const int64_t p = p0 + (int64_t)it * LD_WAVES * R;
        const bool live = p < P;                                   // (a dead position is all zeros: it adds 0)
        const int64_t base = p * C4;
        const float4 a0 = live && has0 ? fa[base + q0] : zero, b0 = live && has0 ? fb[base + q0] : zero;
        const float4 a1 = live && has1 ? fa[base + q1] : zero, b1 = live && has1 ? fb[base + q1] : zero;
        float na = ld_sq(a0) + ld_sq(a1), nb = ld_sq(b0) + ld_sq(b1);
        for (int o = G >> 1; o > 0; o >>= 1) {
            na += __shfl_xor(na, o);
            nb += __shfl_xor(nb, o);
        }
        const float ia = 1.f / (sqrtf(na) + LD_EPS), ib = 1.f / (sqrtf(nb) + LD_EPS);
        acc += (double)(ld_term(a0, ia, b0, ib, w0) + ld_term(a1, ia, b1, ib, w1));
    }
    acc = wave_sum(acc);
    if (lane == 0) wave_d[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < LD_WAVES; ++k) sum += wave_d[k];
        partials[blockIdx.x] = sum;
    }
}

}  // namespace gsdd

using namespace gsdd;

extern "C" int gsdd_lpips_stem_rows(const void* x, int form, int B, int T, int H, int W, int64_t frame0, int64_t n, int padw,
                                    const float* table, float* out, void* stream) {
    GSDD_CHECK_ARG(x && table && out, "null pointer");
    GSDD_CHECK_ARG(form == 0 || form == 1, "form is 0 (float32 planar, normalised) or 1 (uint8 interleaved)");
    GSDD_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0, "bad sizes");
    GSDD_CHECK_ARG(padw >= 0 && padw <= LP_MAX_PADW, "padw is 0 .. 64");
    GSDD_CHECK_ARG(frame0 >= 0 && n > 0 && frame0 <= (int64_t)B * T - n, "frames frame0 .. frame0 + n - 1 must lie inside the B T frames");
    GSDD_CHECK_ARG((form == 1 || (reinterpret_cast<uintptr_t>(x) & 3u) == 0) && (reinterpret_cast<uintptr_t>(table) & 3u) == 0 &&
                       aligned16(out),
                   "a float operand and the table must be 4-byte aligned, out 16-byte aligned");
    GSDD_CHECK_ARG((int64_t)H * W < (1ll << 31) && (int64_t)B * T < (1ll << 31), "a frame holds fewer than 2^31 pixels, a clip set fewer frames");
    const int64_t Wp = (int64_t)W + 2 * padw;
    GSDD_CHECK_ARG(Wp < (1ll << 31) && n <= ((1ll << 31) - 1) * LP_THREADS / (Wp * H), "too many workgroups");
    const int64_t total = n * H * Wp;
    hipLaunchKernelGGL(lpips_stem_rows_kernel, dim3((unsigned)((total + LP_THREADS - 1) / LP_THREADS)), dim3(LP_THREADS), 0,
                       (hipStream_t)stream, x, form, T, H, W, frame0, padw, total, table, GIF_NORM, reinterpret_cast<float4*>(out));
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int64_t gsdd_lpips_distance_slots(int64_t P, int C) {
    if (P < 1 || C < 4 || C > LD_MAX_C || C % 4 != 0) {
        set_error("gsdd_lpips_distance_slots: P >= 1 and C a multiple of 4 in 4 .. 512");
        return GSDD_E_ARG;
    }
    const int64_t rows = ld_rows_per_group(C);
    return (P + rows - 1) / rows;
}

extern "C" int gsdd_lpips_layer_distance(const float* feat, const float* w, int64_t n, int64_t P, int C, double* partials, void* stream) {
    GSDD_CHECK_ARG(feat && w && partials, "null pointer");
    GSDD_CHECK_ARG(C >= 4 && C <= LD_MAX_C && C % 4 == 0, "C is a multiple of 4 in 4 .. 512");
    GSDD_CHECK_ARG(n >= 1 && P >= 1, "bad sizes");
    GSDD_CHECK_ARG(aligned16(feat) && aligned16(w) && (reinterpret_cast<uintptr_t>(partials) & 7u) == 0,
                   "feat and w must be 16-byte aligned, partials 8-byte aligned");
    GSDD_CHECK_ARG(P < (1ll << 31) && n < (1ll << 30) && 2 * n * P < (1ll << 31), "more than 2^31 rows");
    const int64_t rows = ld_rows_per_group(C), slots = (P + rows - 1) / rows;
    GSDD_CHECK_ARG(n * slots < (1ll << 31), "too many workgroups");
    hipLaunchKernelGGL(lpips_layer_distance_kernel, dim3((unsigned)(n * slots)), dim3(LD_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(feat), reinterpret_cast<const float4*>(w), n, P, C / 4, ld_group(C), (int)slots,
                       partials);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}
