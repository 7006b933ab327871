// What the GIF quantiser's device files (gif.hip, gif_refine.hip) share: the uint8 rule, the addressing of a group's pixels, the nearest
// palette entry, and the shape checks of their entries.
#pragma once
#include <cstdint>
#include <string>

#include "common.hpp"

namespace gsdd {

constexpr int64_t GIF_MAX_GROUP_PIXELS = 1ll << 24;            // 255 * 2^24 < 2^32: a box sum cannot overflow

struct GifNorm { float mean[3], std[3]; };

struct GifShape {
    int64_t chan_stride;      // T H W: from one channel plane of a clip to the next
    int64_t group_pixels;     // P
    int64_t frame_pixels;     // H W
    int T, W, per_frame, chunks;
};

__device__ __forceinline__ int gif_level(float x, float mean, float std) {
    const float v = (x * std + mean) * 255.f;
    return (int)fminf(fmaxf(truncf(v), 0.f), 255.f);          // (fmaxf drops a NaN: level 0)
}

// float offset of pixel 0, channel 0 of group g
__device__ __forceinline__ int64_t gif_group_base(const GifShape& s, int64_t g) {
    if (!s.per_frame) return g * 3 * s.chan_stride;
    const int64_t b = g / s.T, t = g - b * s.T;
    return b * 3 * s.chan_stride + t * s.frame_pixels;
}

__device__ __forceinline__ int gif_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the index among pal[0 .. n) (packed R | G << 8 | B << 16, read at a wave-uniform address) of the smallest integer squared distance to
// (r, g, b), the lowest index on ties; 0 with n = 0.  best_d: that distance (0x7fffffff with n = 0)
__device__ __forceinline__ int gif_nearest(const uint32_t* pal, int n, int r, int g, int b, int& best_d) {
    int best = 0;
    best_d = 0x7fffffff;
    for (int i = 0; i < n; ++i) {
        const uint32_t e = pal[i];
        const int dr = r - (int)(e & 255u), dg = g - (int)((e >> 8) & 255u), db = b - (int)((e >> 16) & 255u);
        const int d = dr * dr + dg * dg + db * db;
        if (d < best_d) {                                      // strict: the lowest index wins a tie
            best_d = d;
            best = i;
        }
    }
    return best;
}

static const GifNorm GIF_NORM = {{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}};

// shape checks shared by the entries; chunk = pixels per workgroup.  false = bad arguments (message set)
static bool gif_shape(const char* fn, int B, int T, int H, int W, int per_frame, int chunk, GifShape& s, int64_t& G, int64_t& grid) {
    const auto bad = [&](const char* msg) {
        set_error(std::string(fn) + ": " + msg);
        return false;
    };
    if (B <= 0 || T <= 0 || H <= 0 || W <= 0) return bad("bad sizes");
    if (H > 65535 || W > 65535) return bad("H and W are at most 65535 (a GIF's limit)");
    if (per_frame != 0 && per_frame != 1) return bad("per_frame is 0 or 1");
    if ((int64_t)B * T >= (1ll << 31)) return bad("too many frames");
    s.frame_pixels = (int64_t)H * W;
    s.chan_stride = s.frame_pixels * T;
    s.group_pixels = per_frame ? s.frame_pixels : s.chan_stride;
    if (s.group_pixels > GIF_MAX_GROUP_PIXELS) return bad("a group (clip, or frame with per_frame) holds at most 2^24 pixels");
    s.T = T;
    s.W = W;
    s.per_frame = per_frame;
    s.chunks = (int)((s.group_pixels + chunk - 1) / chunk);
    G = per_frame ? (int64_t)B * T : B;
    grid = G * s.chunks;
    if (grid >= (1ll << 31)) return bad("too many workgroups");
    return true;
}

}  // namespace gsdd
