// Paired video metrics: per (clip, frame, channel) plane the squared error and the SSIM of two clips' uint8 levels (metrics.py's
// paired_frame_metrics; the rule in full: include/gsdd.h).  gif_device.hpp holds the uint8 rule.
//
//   paired   one workgroup of 256 threads owns one PM_TILE x PM_TILE tile of window positions of one plane.  It forms the levels of
//            the tile plus the 10-pixel halo of both operands -- a float is read through the uint8 rule, a byte as it is -- and keeps
//            them in LDS as doubles, zeros beyond the plane.  While staging, a thread adds (a - b)^2 of the pixels its tile OWNS to
//            an integer: the tile's own 16 x 16 pixels, and the halo too in the last tile of a row or column of tiles, so that every
//            pixel of the plane has one owner.  SSIM then takes two separable passes in fp64: along x the 11-tap sums of a, b, a a,
//            b b and a b for the 26 rows x 16 columns the tile needs (LDS), along y the same 11 taps for the thread's own window.
//            Levels are integers below 2^8 and the weights have 24 bits, so every product is exact and a sum of 121 of them carries
//            a relative error of a few 2^-53: E[x x] - mu mu, hopeless in fp32 at x = 250, is good to 1e-10 here, far inside what the
//            centred fp32 form reaches.  gfx950 issues v_fma_f64 / v_mul_f64 / v_add_f64 at the fp32 rate.
//            A's and B's moments come from the same expressions in the same order: equal operands give equal bits, s = 1.0.
//            The windows' s are summed in fp64 over the wave (xor butterfly) and the four waves (in order), rounded to fp32 once, and
//            written with the integer next to it: partials[plane][tile] = {sse, bits of the fp32 sum}.  No atomics, nothing to zero,
//            the same bits in every run.  The SSE-only form (SSIM = false) stops behind the staging loop and uses no LDS but the
//            reduction's.
#include "common.hpp"
#include "gif_device.hpp"

namespace gsdd {

constexpr int PM_TILE = 16, PM_THREADS = PM_TILE * PM_TILE, PM_TAPS = 11, PM_HALO = PM_TAPS - 1, PM_STAGE = PM_TILE + PM_HALO;

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, normalised in fp64 and rounded to fp32: the contract's eleven values (include/gsdd.h)
struct PmWindow { float g[PM_TAPS]; };
static const PmWindow PM_WINDOW = {{0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,
                                    0x1.b43c4p-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}};

struct PmOperand {
    const void* p;
    int form;                 // 0: float32 planar [B][3][T][H][W] through the uint8 rule, 1: uint8 interleaved [B][T][H][W][3]
};

__host__ __device__ inline int64_t pm_tiles_1d(int n) { return n <= PM_HALO + PM_TILE ? 1 : ((int64_t)n - PM_HALO + PM_TILE - 1) / PM_TILE; }

// level of pixel `pix` (y W + x) of plane (b, t, c)
__device__ __forceinline__ int pm_level(const PmOperand& o, int64_t b, int64_t t, int c, int64_t T, int64_t HW, int64_t pix,
                                        const GifNorm& nm) {
    if (o.form == 0) return gif_level(static_cast<const float*>(o.p)[((b * 3 + c) * T + t) * HW + pix], nm.mean[c], nm.std[c]);
    return (int)static_cast<const uint8_t*>(o.p)[((b * T + t) * HW + pix) * 3 + c];
}

template <bool SSIM>
__global__ __launch_bounds__(PM_THREADS) void paired_metrics_kernel(PmOperand A, PmOperand B, int T, int H, int W, int tiles_x, int tiles,
                                                                    GifNorm nm, PmWindow win, int32_t* __restrict__ partials) {
    __shared__ double la[SSIM ? PM_STAGE : 1][PM_STAGE], lb[SSIM ? PM_STAGE : 1][PM_STAGE];
    __shared__ double row[SSIM ? 5 : 1][SSIM ? PM_STAGE : 1][PM_TILE];              // 11-tap sums along x of a, b, a a, b b, a b
    __shared__ double wave_s[PM_THREADS / WAVE];
    __shared__ uint32_t wave_e[PM_THREADS / WAVE];
    const int tid = threadIdx.x;
    const int64_t plane = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - plane * tiles);
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const int y0 = tile_y * PM_TILE, x0 = tile_x * PM_TILE;
    const bool last_y = tile_y == tiles / tiles_x - 1, last_x = tile_x == tiles_x - 1;
    const int c = (int)(plane % 3);
    const int64_t frame = plane / 3, b = frame / T, t = frame - b * T;
    const int64_t HW = (int64_t)H * W;

    uint32_t err = 0u;                                         // at most 26 * 26 * 255^2 < 2^26 in a tile
    for (int i = tid; i < PM_STAGE * PM_STAGE; i += PM_THREADS) {
        const int r = i / PM_STAGE, q = i - r * PM_STAGE;
        const int y = y0 + r, x = x0 + q;
        int va = 0, vb = 0;
        if (y < H && x < W) {
            const int64_t pix = (int64_t)y * W + x;
            va = pm_level(A, b, t, c, T, HW, pix, nm);
            vb = pm_level(B, b, t, c, T, HW, pix, nm);
            if ((r < PM_TILE || last_y) && (q < PM_TILE || last_x)) err += (uint32_t)((va - vb) * (va - vb));
        }
        if constexpr (SSIM) {
            la[r][q] = (double)va;
            lb[r][q] = (double)vb;
        }
    }

    double s = 0.0;
    if constexpr (SSIM) {
        double g[PM_TAPS];
#pragma unroll
        for (int j = 0; j < PM_TAPS; ++j) g[j] = (double)win.g[j];
        __syncthreads();
        for (int i = tid; i < PM_STAGE * PM_TILE; i += PM_THREADS) {
            const int r = i / PM_TILE, q = i - r * PM_TILE;
            double ha = 0.0, hb = 0.0, haa = 0.0, hbb = 0.0, hab = 0.0;
#pragma unroll
            for (int j = 0; j < PM_TAPS; ++j) {
                const double a = la[r][q + j], bb = lb[r][q + j];
                ha += g[j] * a;
                hb += g[j] * bb;
                haa += g[j] * (a * a);
                hbb += g[j] * (bb * bb);
                hab += g[j] * (a * bb);
            }
            row[0][r][q] = ha;
            row[1][r][q] = hb;
            row[2][r][q] = haa;
            row[3][r][q] = hbb;
            row[4][r][q] = hab;
        }
        __syncthreads();
        const int wy = tid / PM_TILE, wx = tid - wy * PM_TILE;
        double ma = 0.0, mb = 0.0, eaa = 0.0, ebb = 0.0, eab = 0.0;
#pragma unroll
        for (int j = 0; j < PM_TAPS; ++j) {
            ma += g[j] * row[0][wy + j][wx];
            mb += g[j] * row[1][wy + j][wx];
            eaa += g[j] * row[2][wy + j][wx];
            ebb += g[j] * row[3][wy + j][wx];
            eab += g[j] * row[4][wy + j][wx];
        }
        constexpr double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
        // moments ABOUT the means with weights that sum to sw = (sum g)^2 = 1 - 2.8e-9, not to 1 (the rule divides by nothing):
        // sum w (a - ma)(b - mb) = sum w a b - (2 - sw) ma mb
        double sg = 0.0;
#pragma unroll
        for (int j = 0; j < PM_TAPS; ++j) sg += g[j];
        const double k = 2.0 - sg * sg;
        const double saa = eaa - k * (ma * ma), sbb = ebb - k * (mb * mb), sab = eab - k * (ma * mb);
        const double num = (2.0 * (ma * mb) + C1) * (2.0 * sab + C2);
        const double den = ((ma * ma + mb * mb) + C1) * ((saa + sbb) + C2);
        if (y0 + wy <= H - PM_TAPS && x0 + wx <= W - PM_TAPS) s = num / den;       // (a window beyond the plane: 0 to the sum)
        s = wave_sum(s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) err += (uint32_t)__shfl_xor((int)err, o);
    if ((tid & (WAVE - 1)) == 0) {
        wave_s[tid / WAVE] = s;
        wave_e[tid / WAVE] = err;
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        uint32_t e = 0u;
#pragma unroll
        for (int w = 0; w < PM_THREADS / WAVE; ++w) {
            sum += wave_s[w];
            e += wave_e[w];
        }
        int32_t* out = partials + 2 * (int64_t)blockIdx.x;
        out[0] = (int32_t)e;
        out[1] = __float_as_int((float)sum);
    }
}

}  // namespace gsdd

using namespace gsdd;

extern "C" int64_t gsdd_paired_metrics_tiles(int H, int W) {
    if (H <= 0 || W <= 0) {
        set_error("gsdd_paired_metrics_tiles: bad sizes");
        return GSDD_E_ARG;
    }
    return pm_tiles_1d(H) * pm_tiles_1d(W);
}

extern "C" int gsdd_paired_metrics(const void* a, int form_a, const void* b, int form_b, int B, int T, int H, int W, int want_ssim,
                                   int32_t* partials, void* stream) {
    GSDD_CHECK_ARG(a && b && partials, "null pointer");
    GSDD_CHECK_ARG((form_a == 0 || form_a == 1) && (form_b == 0 || form_b == 1),
                   "a form is 0 (float32 planar, normalised) or 1 (uint8 interleaved)");
    GSDD_CHECK_ARG(want_ssim == 0 || want_ssim == 1, "want_ssim is 0 or 1");
    GSDD_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0, "bad sizes");
    GSDD_CHECK_ARG(!want_ssim || (H >= PM_TAPS && W >= PM_TAPS), "SSIM needs H and W of at least 11 (one 11 x 11 window)");
    GSDD_CHECK_ARG((form_a == 1 || (reinterpret_cast<uintptr_t>(a) & 3u) == 0) && (form_b == 1 || (reinterpret_cast<uintptr_t>(b) & 3u) == 0) &&
                       (reinterpret_cast<uintptr_t>(partials) & 3u) == 0,
                   "float operands and partials must be 4-byte aligned");
    GSDD_CHECK_ARG((int64_t)H * W < (1ll << 31), "a plane holds fewer than 2^31 pixels");
    const int64_t planes = (int64_t)B * T * 3;
    const int64_t tiles_x = pm_tiles_1d(W), tiles = pm_tiles_1d(H) * tiles_x;
    GSDD_CHECK_ARG(planes < (1ll << 31) && tiles < (1ll << 31) && planes * tiles < (1ll << 31), "too many workgroups");
    const auto kernel = want_ssim ? paired_metrics_kernel<true> : paired_metrics_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(planes * tiles)), dim3(PM_THREADS), 0, (hipStream_t)stream, PmOperand{a, form_a},
                       PmOperand{b, form_b}, T, H, W, (int)tiles_x, (int)tiles, GIF_NORM, PM_WINDOW, partials);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}
