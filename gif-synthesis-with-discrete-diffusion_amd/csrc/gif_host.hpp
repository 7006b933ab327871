// Host half of the GIF export: the median cut over a 15-bit colour histogram and the GIF89a / LZW writer.  Plain C++ (no HIP, nothing
// of common.hpp): csrc/gif.hip wraps these in the C ABI, and a stand-alone program can include the header as it is.
//
// Median cut.  A bin is (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3).  Integer only and deterministic: one box with every occupied bin;
// while there are fewer than `colors` boxes, the box with the largest pixel count among those with more than one occupied bin (ties:
// lowest index) is cut along its axis of largest extent in bin coordinates (the tight bounds of its occupied bins; ties R, G, B)
// after the first plane where twice the cumulative count reaches the box total -- one plane earlier if that is the last plane, so
// both parts are non-empty.  The lower part keeps the index, the upper part is appended.  Unoccupied bins map to 255.
//
// Writer.  Header, logical screen descriptor, a global colour table (one palette) or local ones (one palette per frame), each padded
// with zeros to a power of two of at least 2 entries; the NETSCAPE2.0 loop extension; per frame a graphic control extension
// (disposal 1, the delay), an image descriptor and the LZW stream in sub-blocks of at most 255 bytes; the trailer.  LZW: minimum code
// size max(2, bits), a clear code first, codes growing to 12 bits, a clear code and a table reset when the table holds 4096 entries,
// the end-of-information code.  encode() writes whole frames without transparency; encode_delta() writes each frame's rectangle of
// changed pixels with a transparent index for the pixels that keep their colour (the delta stage: csrc/gif_delta.hip).  Nothing is ever
// written at or behind out[cap].
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

namespace gsdd {
namespace gif {

constexpr int BINS = 32768;

// -> the number of boxes (0 for an empty histogram); box_of_bin[bin] = the box of an occupied bin, 255 for an unoccupied one
inline int median_cut(const uint32_t* hist, int colors, uint8_t* box_of_bin) {
    struct Box { int begin, end; uint64_t count; };          // bins[begin .. end): the occupied bins of the box
    std::vector<int> bins;
    uint64_t total = 0;
    for (int i = 0; i < BINS; ++i)
        if (hist[i] != 0u) {
            bins.push_back(i);
            total += hist[i];
        }
    memset(box_of_bin, 255, BINS);
    if (bins.empty()) return 0;
    std::vector<Box> boxes;
    boxes.push_back({0, (int)bins.size(), total});
    std::vector<int> lower, upper;
    while ((int)boxes.size() < colors) {
        int pick = -1;
        for (int i = 0; i < (int)boxes.size(); ++i)
            if (boxes[i].end - boxes[i].begin > 1 && (pick < 0 || boxes[i].count > boxes[pick].count)) pick = i;
        if (pick < 0) break;
        const Box bx = boxes[pick];
        int lo[3] = {31, 31, 31}, hi[3] = {0, 0, 0};
        for (int i = bx.begin; i < bx.end; ++i)
            for (int a = 0; a < 3; ++a) {
                const int v = (bins[i] >> (10 - 5 * a)) & 31;
                if (v < lo[a]) lo[a] = v;
                if (v > hi[a]) hi[a] = v;
            }
        int axis = 0;
        for (int a = 1; a < 3; ++a)
            if (hi[a] - lo[a] > hi[axis] - lo[axis]) axis = a;
        const int shift = 10 - 5 * axis;
        uint64_t plane[32] = {0};
        for (int i = bx.begin; i < bx.end; ++i) plane[(bins[i] >> shift) & 31] += hist[bins[i]];
        int cut = lo[axis];
        uint64_t cum = 0;
        for (; cut <= hi[axis]; ++cut) {
            cum += plane[cut];
            if (2 * cum >= bx.count) break;
        }
        if (cut >= hi[axis]) cut = hi[axis] - 1;                 // (extent > 0: more than one occupied bin)
        lower.clear();
        upper.clear();
        uint64_t lower_count = 0;
        for (int i = bx.begin; i < bx.end; ++i) {
            if (((bins[i] >> shift) & 31) <= cut) {
                lower.push_back(bins[i]);
                lower_count += hist[bins[i]];
            } else {
                upper.push_back(bins[i]);
            }
        }
        int w = bx.begin;
        for (int b : lower) bins[w++] = b;
        const int mid = w;
        for (int b : upper) bins[w++] = b;
        boxes[pick] = {bx.begin, mid, lower_count};
        boxes.push_back({mid, bx.end, bx.count - lower_count});
    }
    for (int i = 0; i < (int)boxes.size(); ++i)
        for (int j = boxes[i].begin; j < boxes[i].end; ++j) box_of_bin[bins[j]] = (uint8_t)i;
    return (int)boxes.size();
}

// bits of a colour table with n entries: the table holds 1 << bits >= max(n, 2) colours
inline int table_bits(int n) {
    int bits = 1;
    while ((1 << bits) < n) ++bits;
    return bits;
}

// an upper bound of what encode() writes: 1.5 bytes per pixel at 12 bits a code, the clear codes, the sub-block lengths and the
// per-frame and per-file headers with full colour tables
inline int64_t encode_bound(int64_t T, int64_t H, int64_t W) { return 832 + T * (896 + 2 * H * W); }

struct Writer {
    uint8_t* out;
    int64_t cap, pos;
    void put(uint8_t b) {
        if (pos < cap) out[pos] = b;
        ++pos;
    }
    void put16(int v) {
        put((uint8_t)(v & 255));
        put((uint8_t)((v >> 8) & 255));
    }
    void bytes(const void* p, int n) {
        for (int i = 0; i < n; ++i) put(static_cast<const uint8_t*>(p)[i]);
    }
    void table(const uint8_t* rgb, int n, int bits) {
        for (int i = 0; i < (1 << bits); ++i)
            for (int c = 0; c < 3; ++c) put(i < n ? rgb[3 * i + c] : (uint8_t)0);
    }
};

// the LZW stream of one frame in sub-blocks; -> the clear codes emitted
inline int64_t lzw_frame(Writer& w, const uint8_t* px, int64_t n, int min_code) {
    constexpr int HASH = 8192;                                // open addressing over at most 4096 - 6 entries
    std::vector<int32_t> key(HASH);
    std::vector<int16_t> val(HASH);
    uint8_t block[255];
    int fill = 0;
    uint32_t acc = 0;
    int nbits = 0;
    const int clear = 1 << min_code, eoi = clear + 1;
    int next = clear + 2, width = min_code + 1;
    int64_t clears = 0;
    auto emit = [&](int code) {
        acc |= (uint32_t)code << nbits;
        nbits += width;
        while (nbits >= 8) {
            block[fill++] = (uint8_t)(acc & 255u);
            acc >>= 8;
            nbits -= 8;
            if (fill == 255) {
                w.put(255);
                w.bytes(block, 255);
                fill = 0;
            }
        }
    };
    auto reset = [&]() {
        emit(clear);
        ++clears;
        for (int i = 0; i < HASH; ++i) key[i] = -1;
        next = clear + 2;
        width = min_code + 1;
    };
    reset();
    int prefix = px[0];
    for (int64_t i = 1; i < n; ++i) {
        const int c = px[i];
        const int32_t k = (prefix << 8) | c;
        int h = (int)(((uint32_t)k * 2654435761u) >> 19);   // 13 bits
        while (key[h] != -1 && key[h] != k) h = (h + 1) & (HASH - 1);
        if (key[h] == k) {
            prefix = val[h];
            continue;
        }
        emit(prefix);
        key[h] = k;
        val[h] = (int16_t)next;
        ++next;
        if (next > (1 << width) && width < 12) ++width;
        if (next == 4096) reset();
        prefix = c;
    }
    emit(prefix);
    ++next;                                                   // the entry the decoder adds on this code: it may widen the next one
    if (next > (1 << width) && width < 12) ++width;
    emit(eoi);
    if (nbits > 0) block[fill++] = (uint8_t)(acc & 255u);
    if (fill > 0) {
        w.put((uint8_t)fill);
        w.bytes(block, fill);
    }
    w.put(0);
    return clears;
}

constexpr int64_t E_ARG = -1, E_CAP = -4;

// indices [T][H][W]; palettes [n_palettes][256][3] with n_colors[n_palettes], n_palettes 1 (a global table) or T (local tables);
// -> bytes written, E_ARG for bad arguments (an index outside its table included), E_CAP when cap is too small
inline int64_t encode(const uint8_t* indices, int T, int H, int W, const uint8_t* palettes, const int32_t* n_colors, int n_palettes,
                      int delay_cs, int loop, uint8_t* out, int64_t cap, int64_t* clear_codes) {
    if (!indices || !palettes || !n_colors || !out) return E_ARG;
    if (T <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || cap < 0) return E_ARG;
    if ((n_palettes != 1 && n_palettes != T) || delay_cs < 0 || delay_cs > 65535 || loop < 0 || loop > 65535) return E_ARG;
    for (int p = 0; p < n_palettes; ++p)
        if (n_colors[p] < 1 || n_colors[p] > 256) return E_ARG;
    const int64_t n = (int64_t)H * W;
    const bool local = n_palettes > 1;
    for (int t = 0; t < T; ++t) {
        const int nc = n_colors[local ? t : 0];
        const uint8_t* px = indices + t * n;
        for (int64_t i = 0; i < n; ++i)
            if (px[i] >= nc) return E_ARG;
    }
    Writer w = {out, cap, 0};
    w.bytes("GIF89a", 6);
    w.put16(W);
    w.put16(H);
    const int gbits = table_bits(n_colors[0]);
    w.put(local ? (uint8_t)0x70 : (uint8_t)(0x80 | 0x70 | (gbits - 1)));
    w.put(0);
    w.put(0);
    if (!local) w.table(palettes, n_colors[0], gbits);
    w.put(0x21);
    w.put(0xFF);
    w.put(11);
    w.bytes("NETSCAPE2.0", 11);
    w.put(3);
    w.put(1);
    w.put16(loop);
    w.put(0);
    int64_t clears = 0;
    for (int t = 0; t < T; ++t) {
        const int p = local ? t : 0;
        const int bits = table_bits(n_colors[p]);
        w.put(0x21);
        w.put(0xF9);
        w.put(4);
        w.put(1 << 2);                                        // disposal 1 (leave in place), no transparency
        w.put16(delay_cs);
        w.put(0);
        w.put(0);
        w.put(0x2C);
        w.put16(0);
        w.put16(0);
        w.put16(W);
        w.put16(H);
        w.put(local ? (uint8_t)(0x80 | (bits - 1)) : (uint8_t)0);
        if (local) w.table(palettes + (int64_t)p * 768, n_colors[p], bits);
        const int min_code = bits < 2 ? 2 : bits;
        w.put((uint8_t)min_code);
        clears += lzw_frame(w, indices + t * n, n, min_code);
    }
    w.put(0x3B);
    if (clear_codes) *clear_codes = clears;
    return w.pos <= cap ? w.pos : E_CAP;
}

// encode() for delta frames (gsdd_gif_delta's outputs): frame t is the sub-image rects[t] = x0, y0, x1, y1 (inclusive) of the full-frame
// indices [T][H][W], read at stride W; the empty marker (W, H, -1, -1) is written as the 1 x 1 image at (0, 0).  transparent[n_palettes]:
// the transparent index of each table's frames, -1 = none; a table covers it (max(n_colors, transparent + 1) entries before the
// padding) and the graphic control extension names it.  Disposal 1, the LZW writer of encode(); encode_bound() holds.  E_ARG as
// encode(), and for a rectangle that leaves the canvas or is inverted, a transparent index outside -1 .. 255 and an index of a
// rectangle that is neither in front of n_colors nor the transparent one.
inline int64_t encode_delta(const uint8_t* indices, int T, int H, int W, const uint8_t* palettes, const int32_t* n_colors, int n_palettes,
                            const int32_t* rects, const int32_t* transparent, int delay_cs, int loop, uint8_t* out, int64_t cap,
                            int64_t* clear_codes) {
    if (!indices || !palettes || !n_colors || !rects || !transparent || !out) return E_ARG;
    if (T <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || cap < 0) return E_ARG;
    if ((n_palettes != 1 && n_palettes != T) || delay_cs < 0 || delay_cs > 65535 || loop < 0 || loop > 65535) return E_ARG;
    for (int p = 0; p < n_palettes; ++p)
        if (n_colors[p] < 1 || n_colors[p] > 256 || transparent[p] < -1 || transparent[p] > 255) return E_ARG;
    const int64_t n = (int64_t)H * W;
    const bool local = n_palettes > 1;
    struct Rect { int x, y, w, h; };
    std::vector<Rect> boxes((size_t)T);
    for (int t = 0; t < T; ++t) {
        const int32_t* r = rects + 4 * (int64_t)t;
        if (r[0] == W && r[1] == H && r[2] == -1 && r[3] == -1) {
            boxes[t] = {0, 0, 1, 1};
        } else {
            if (r[0] < 0 || r[1] < 0 || r[2] < r[0] || r[3] < r[1] || r[2] >= W || r[3] >= H) return E_ARG;
            boxes[t] = {r[0], r[1], r[2] - r[0] + 1, r[3] - r[1] + 1};
        }
        const int nc = n_colors[local ? t : 0], tr = transparent[local ? t : 0];
        for (int y = 0; y < boxes[t].h; ++y) {
            const uint8_t* px = indices + t * n + (int64_t)(boxes[t].y + y) * W + boxes[t].x;
            for (int x = 0; x < boxes[t].w; ++x)
                if (px[x] >= nc && px[x] != tr) return E_ARG;
        }
    }
    const auto entries = [&](int p) { return n_colors[p] > transparent[p] + 1 ? n_colors[p] : transparent[p] + 1; };
    Writer w = {out, cap, 0};
    w.bytes("GIF89a", 6);
    w.put16(W);
    w.put16(H);
    const int gbits = table_bits(entries(0));
    w.put(local ? (uint8_t)0x70 : (uint8_t)(0x80 | 0x70 | (gbits - 1)));
    w.put(0);
    w.put(0);
    if (!local) w.table(palettes, n_colors[0], gbits);
    w.put(0x21);
    w.put(0xFF);
    w.put(11);
    w.bytes("NETSCAPE2.0", 11);
    w.put(3);
    w.put(1);
    w.put16(loop);
    w.put(0);
    int64_t clears = 0;
    std::vector<uint8_t> rows;
    for (int t = 0; t < T; ++t) {
        const int p = local ? t : 0;
        const int bits = table_bits(entries(p));
        const int tr = transparent[p];
        const Rect& bx = boxes[t];
        w.put(0x21);
        w.put(0xF9);
        w.put(4);
        w.put((uint8_t)((1 << 2) | (tr >= 0 ? 1 : 0)));       // disposal 1 (leave in place), the transparency flag
        w.put16(delay_cs);
        w.put((uint8_t)(tr >= 0 ? tr : 0));
        w.put(0);
        w.put(0x2C);
        w.put16(bx.x);
        w.put16(bx.y);
        w.put16(bx.w);
        w.put16(bx.h);
        w.put(local ? (uint8_t)(0x80 | (bits - 1)) : (uint8_t)0);
        if (local) w.table(palettes + (int64_t)p * 768, n_colors[p], bits);
        const int min_code = bits < 2 ? 2 : bits;
        w.put((uint8_t)min_code);
        rows.resize((size_t)bx.w * bx.h);
        for (int y = 0; y < bx.h; ++y) memcpy(rows.data() + (size_t)y * bx.w, indices + t * n + (int64_t)(bx.y + y) * W + bx.x, (size_t)bx.w);
        clears += lzw_frame(w, rows.data(), (int64_t)bx.w * bx.h, min_code);
    }
    w.put(0x3B);
    if (clear_codes) *clear_codes = clears;
    return w.pos <= cap ? w.pos : E_CAP;
}

}  // namespace gif
}  // namespace gsdd
