// GIF export, between the quantiser and the encoder: the delta stage.  A pixel that shows the same colour as the frame before it (or one
// within a tolerance of what it should show) is written as the frame's transparent index, and every frame gets the bounding box of the
// pixels that did change, so that gsdd_gif_encode_delta (gif_host.hpp) writes sub-rectangles with transparent pixels instead of whole
// frames.  gif_device.hpp holds the uint8 rule and the groups; the rule of this stage in full: include/gsdd.h.
//
//   delta   one thread owns GIFD_PIX = 4 consecutive pixels of the flat H W canvas of one clip and walks its T frames with `shown`, the
//           colour each of them displays, in registers -- the compositor's shape (gif_read.hip), run the other way.  Indices are read
//           and written as one dword per thread and frame; a slot whose first byte is not dword aligned (H W odd: every other frame)
//           goes bytewise, as do the last H W mod 4 pixels of the canvas.  The palette entry of an index is read from global memory (1 KB
//           per group: it stays in the caches), n_colors at an address that depends on the loop counter alone.  The tolerance form
//           (TOL) also reads the pixel's three floats, as one float4 per channel where the slot allows; the exact form never touches
//           `clips`.  Rectangles and counts are reduced per workgroup in LDS -- [5][GIFD_FRAMES] words: min x, min y, max x, max y,
//           count -- with LDS atomics by the threads that saw a change, and flushed with global integer min / max / add atomics for
//           the frames the workgroup changed something in.  T above GIFD_FRAMES runs in chunks of GIFD_FRAMES frames with a flush
//           behind each; `shown` lives on across them.  Integer results: exact, whatever order the workgroups run in.
// rects and changed are initialised by the same kernel in an `init` launch (a kernel, not a memset node: DESIGN section 9).
#include <algorithm>

#include "common.hpp"
#include "gif_device.hpp"
#include "gif_host.hpp"

namespace gsdd {

constexpr int GIFD_THREADS = 256, GIFD_PIX = 4, GIFD_CHUNK = GIFD_THREADS * GIFD_PIX;
constexpr int GIFD_FRAMES = GIFD_THREADS;                      // frames per LDS table: thread i initialises and flushes frame i
constexpr int GIF_MAX_TOLERANCE = 3 * 255 * 255;

template <bool TOL>
__global__ __launch_bounds__(GIFD_THREADS) void gif_delta_kernel(const float* __restrict__ clips, const uint8_t* __restrict__ indices,
                                                                 GifShape s, GifNorm nm, int H, int frame_chunks,
                                                                 const uint32_t* __restrict__ palette, const int32_t* __restrict__ n_colors,
                                                                 int tolerance, uint8_t* __restrict__ out, int32_t* __restrict__ rects,
                                                                 uint32_t* __restrict__ changed, int64_t init_frames) {
    __shared__ int box[5][GIFD_FRAMES];
    const int W = s.W, T = s.T;
    if (init_frames) {                                         // the init launch: rects = (W, H, -1, -1), changed = 0
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < init_frames; i += (int64_t)gridDim.x * blockDim.x) {
            rects[4 * i + 0] = W;
            rects[4 * i + 1] = H;
            rects[4 * i + 2] = -1;
            rects[4 * i + 3] = -1;
            changed[i] = 0u;
        }
        return;
    }
    const int64_t HW = s.frame_pixels;
    const int64_t b = blockIdx.x / frame_chunks;
    const int64_t p0 = ((int64_t)(blockIdx.x - b * frame_chunks) * GIFD_THREADS + threadIdx.x) * GIFD_PIX;
    const int npx = p0 >= HW ? 0 : (HW - p0 < GIFD_PIX ? (int)(HW - p0) : GIFD_PIX);        // 0: beyond the canvas (barriers: no return)
    int xs[GIFD_PIX], ys[GIFD_PIX];
    ys[0] = (int)(p0 / W);
    xs[0] = (int)(p0 - (int64_t)ys[0] * W);
#pragma unroll
    for (int i = 1; i < GIFD_PIX; ++i) {
        const bool wrap = xs[i - 1] + 1 == W;
        xs[i] = wrap ? 0 : xs[i - 1] + 1;
        ys[i] = ys[i - 1] + (wrap ? 1 : 0);
    }
    uint32_t shown[GIFD_PIX] = {0u, 0u, 0u, 0u};
    for (int t0 = 0; t0 < T; t0 += GIFD_FRAMES) {
        const int nt = T - t0 < GIFD_FRAMES ? T - t0 : GIFD_FRAMES;
        box[0][threadIdx.x] = W;
        box[1][threadIdx.x] = H;
        box[2][threadIdx.x] = -1;
        box[3][threadIdx.x] = -1;
        box[4][threadIdx.x] = 0;
        __syncthreads();
        for (int k = 0; k < nt && npx > 0; ++k) {
            const int t = t0 + k;
            const int64_t f = b * T + t;
            const int64_t g = s.per_frame ? f : b;
            const int n = n_colors[g];
            const int transparent = n < 256 ? n : -1;
            const uint32_t* pal = palette + g * 256;
            const uint8_t* src = indices + f * HW + p0;
            uint8_t* dst = out + f * HW + p0;
            const bool whole = npx == GIFD_PIX && (reinterpret_cast<uintptr_t>(src) & 3u) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0;
            int idx[GIFD_PIX];
            if (whole) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(src);
#pragma unroll
                for (int i = 0; i < GIFD_PIX; ++i) idx[i] = (int)((v >> (8 * i)) & 255u);
            } else {
#pragma unroll
                for (int i = 0; i < GIFD_PIX; ++i) idx[i] = i < npx ? (int)src[i] : 0;
            }
            float x[3][GIFD_PIX];
            if constexpr (TOL) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float* pc = clips + (b * 3 + c) * s.chan_stride + (int64_t)t * HW + p0;
                    if (npx == GIFD_PIX && (reinterpret_cast<uintptr_t>(pc) & 15u) == 0) {
                        const float4 v = *reinterpret_cast<const float4*>(pc);
                        x[c][0] = v.x, x[c][1] = v.y, x[c][2] = v.z, x[c][3] = v.w;
                    } else {
#pragma unroll
                        for (int i = 0; i < GIFD_PIX; ++i) x[c][i] = i < npx ? pc[i] : 0.f;
                    }
                }
            }
            int x0 = W, y0 = H, x1 = -1, y1 = -1, count = 0;
            uint32_t packed = 0u;
#pragma unroll
            for (int i = 0; i < GIFD_PIX; ++i) {
                const uint32_t c = pal[idx[i]] & 0xFFFFFFu;
                bool unchanged = t > 0 && c == shown[i];
                if constexpr (TOL) {
                    const int dr = gif_level(x[0][i], nm.mean[0], nm.std[0]) - (int)(shown[i] & 255u);
                    const int dg = gif_level(x[1][i], nm.mean[1], nm.std[1]) - (int)((shown[i] >> 8) & 255u);
                    const int db = gif_level(x[2][i], nm.mean[2], nm.std[2]) - (int)((shown[i] >> 16) & 255u);
                    unchanged = unchanged || (t > 0 && transparent >= 0 && dr * dr + dg * dg + db * db <= tolerance);
                }
                const int o = unchanged && transparent >= 0 ? transparent : idx[i];
                packed |= (uint32_t)o << (8 * i);
                if (!unchanged) shown[i] = c;
                if (!unchanged && i < npx) {
                    x0 = min(x0, xs[i]);
                    y0 = min(y0, ys[i]);
                    x1 = max(x1, xs[i]);
                    y1 = max(y1, ys[i]);
                    ++count;
                }
            }
            if (whole) {
                *reinterpret_cast<uint32_t*>(dst) = packed;
            } else {
#pragma unroll
                for (int i = 0; i < GIFD_PIX; ++i)
                    if (i < npx) dst[i] = (uint8_t)(packed >> (8 * i));
            }
            if (count) {
                atomicMin(&box[0][k], x0);
                atomicMin(&box[1][k], y0);
                atomicMax(&box[2][k], x1);
                atomicMax(&box[3][k], y1);
                atomicAdd(&box[4][k], count);
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < nt && box[4][threadIdx.x]) {    // only the frames this workgroup changed something in
            const int64_t f = b * T + t0 + threadIdx.x;
            atomicMin(&rects[4 * f + 0], box[0][threadIdx.x]);
            atomicMin(&rects[4 * f + 1], box[1][threadIdx.x]);
            atomicMax(&rects[4 * f + 2], box[2][threadIdx.x]);
            atomicMax(&rects[4 * f + 3], box[3][threadIdx.x]);
            atomicAdd(&changed[f], (uint32_t)box[4][threadIdx.x]);
        }
    }                                                          // (thread i alone touches entry i between the flush and the next chunk's init)
}

}  // namespace gsdd

using namespace gsdd;

extern "C" int gsdd_gif_delta(const float* clips, const uint8_t* indices, int B, int T, int H, int W, int per_frame, const uint8_t* palette,
                              const int32_t* n_colors, int tolerance, uint8_t* out, int32_t* rects, uint32_t* changed, void* stream) {
    GSDD_CHECK_ARG(clips && indices && palette && n_colors && out && rects && changed, "null pointer");
    GSDD_CHECK_ARG((reinterpret_cast<uintptr_t>(palette) & 3u) == 0, "palette must be 4-byte aligned");
    GSDD_CHECK_ARG((reinterpret_cast<uintptr_t>(clips) & 3u) == 0 && (reinterpret_cast<uintptr_t>(rects) & 3u) == 0 &&
                       (reinterpret_cast<uintptr_t>(changed) & 3u) == 0,
                   "clips, rects and changed must be 4-byte aligned");
    GSDD_CHECK_ARG(tolerance >= 0 && tolerance <= GIF_MAX_TOLERANCE, "tolerance is a squared RGB distance in 0 .. 195075");
    GSDD_CHECK_ARG(indices != out, "out must not be indices");
    GifShape s;
    int64_t G, grid;
    if (!gif_shape(__func__, B, T, H, W, per_frame, GIFD_CHUNK, s, G, grid)) return GSDD_E_ARG;
    const int frame_chunks = (int)((s.frame_pixels + GIFD_CHUNK - 1) / GIFD_CHUNK);
    grid = (int64_t)B * frame_chunks;
    GSDD_CHECK_ARG(grid < (1ll << 31), "too many workgroups");
    const int64_t frames = (int64_t)B * T;
    const unsigned igrid = (unsigned)std::min<int64_t>((frames + GIFD_THREADS - 1) / GIFD_THREADS, 1024);
    const uint32_t* pal = reinterpret_cast<const uint32_t*>(palette);
    const auto kernel = tolerance > 0 ? gif_delta_kernel<true> : gif_delta_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(igrid), dim3(GIFD_THREADS), 0, (hipStream_t)stream, clips, indices, s, GIF_NORM, H, frame_chunks, pal,
                       n_colors, tolerance, out, rects, changed, frames);
    GSDD_CHECK_LAUNCH();
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(GIFD_THREADS), 0, (hipStream_t)stream, clips, indices, s, GIF_NORM, H, frame_chunks,
                       pal, n_colors, tolerance, out, rects, changed, (int64_t)0);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

// ---------------------------------------------------------------- host half (HOST pointers; nothing is launched)
extern "C" int64_t gsdd_gif_encode_delta(const uint8_t* indices, int T, int H, int W, const uint8_t* palettes, const int32_t* n_colors,
                                         int n_palettes, const int32_t* rects, const int32_t* transparent, int delay_cs, int loop,
                                         uint8_t* out, int64_t cap, int64_t* clear_codes) {
    const int64_t rc = gif::encode_delta(indices, T, H, W, palettes, n_colors, n_palettes, rects, transparent, delay_cs, loop, out, cap,
                                         clear_codes);
    if (rc == gif::E_ARG) {
        set_error("gsdd_gif_encode_delta: bad argument (null pointer, sizes, n_palettes not 1 or T, n_colors outside 1 .. 256, delay or "
                  "loop outside 0 .. 65535, a rectangle that leaves the canvas or is inverted, a transparent index outside -1 .. 255, or "
                  "an index outside its colour table)");
        return GSDD_E_ARG;
    }
    if (rc == gif::E_CAP) {
        set_error("gsdd_gif_encode_delta: the output buffer is too small (gsdd_gif_encode_bound gives a sufficient size)");
        return GSDD_E_CAP;
    }
    return rc;
}
