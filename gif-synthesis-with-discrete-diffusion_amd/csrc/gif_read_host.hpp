// Host half of the GIF import: the block walk of a GIF87a / GIF89a file and the LZW decoder.  Plain C++ (no HIP, nothing of common.hpp):
// csrc/gif_read.hip wraps these in the C ABI, and a stand-alone program can include the header as it is.  The bytes are FOREIGN: every
// read goes through a bounds check against data[0 .. n), every write through one against the caller's capacity.
//
// Walk.  Header ("GIF87a" / "GIF89a"), logical screen descriptor (W, H in 1 .. 65535), the global colour table if flagged; then blocks
// until the trailer 0x3B or the end of the data (a missing trailer behind a complete frame is accepted):
//   0x21 0xF9   graphic control extension: disposal, transparent index and delay of the NEXT image; disposals 4 .. 7 count as 0
//   0x21 0xFF   application extension: "NETSCAPE2.0" / "ANIMEXTS1.0" with a sub-block (1, lo, hi) gives the loop count
//   0x21 other  skipped
//   0x2C        image: x, y, w, h (inside the canvas, w and h at least 1), a local colour table if flagged, the minimum code size
//               (1 .. 8), the LZW stream in sub-blocks of 1 .. 255 bytes closed by a zero length
// Colour tables become rows of palettes[P][256][4] (R, G, B, 0; zeros behind a table's size) in file order, the global one first.
// A frame is described by 8 plain integers (no struct crosses the ABI): x, y, w, h, raster offset, palette row, transparent index
// (-1 = none), disposal.
//
// LZW.  Codes of min + 1 bits, least significant bit first, growing by one bit when the next free entry reaches 1 << width, at most
// 12 (with a minimum code size of 1 the next free entry is 4 = 1 << 2 from the start: the width grows behind the first code after a
// clear code, as it does in giflib and in this project's writer); the clear code resets table and width; with 4096 entries the table
// stops growing and codes stay 12 bits until a clear arrives (the deferred clear); a code equal to the next free entry is the previous
// string plus its own first pixel (KwKwK).  Decoding of a frame stops at w * h pixels (what a code yields beyond them is dropped,
// later codes are not looked at), at the end code or at the end of the sub-block chain; fewer than w * h pixels is an error.
// Interlaced frames (rows 0, 8, ..; 4, 12, ..; 2, 6, ..; 1, 3, ..) are stored in display order.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

namespace gsdd {
namespace gifr {

constexpr int OK = 0, E_ARG = -1, E_CAP = -4;
constexpr int64_t MAX_RASTER = 2147483647ll;                  // the sum of w * h over all frames stays an int32

struct Error {
    int64_t offset;                                           // the byte the walk stopped at
    const char* what;
};

struct Source {
    const uint8_t* d;
    int64_t n, pos;
    bool has(int64_t k) const { return k <= n - pos; }
    int u8() { return d[pos++]; }
    int u16() {
        const int v = d[pos] | (d[pos + 1] << 8);
        pos += 2;
        return v;
    }
};

// skips a chain of sub-blocks from s.pos; false when the data ends inside it
inline bool skip_chain(Source& s) {
    for (;;) {
        if (!s.has(1)) return false;
        const int len = s.u8();
        if (len == 0) return true;
        if (!s.has(len)) {
            s.pos = s.n;
            return false;
        }
        s.pos += len;
    }
}

// the bytes of a sub-block chain, one at a time
struct Chain {
    Source& s;
    int left;                                                 // bytes left in the open sub-block
    bool closed, cut;                                         // the zero length was read / the data ended inside the chain
    explicit Chain(Source& src) : s(src), left(0), closed(false), cut(false) {}
    // -> the next byte, or -1 at the end of the chain (closed or cut)
    int next() {
        if (closed || cut) return -1;
        if (left == 0) {
            if (!s.has(1)) {
                cut = true;
                return -1;
            }
            left = s.u8();
            if (left == 0) {
                closed = true;
                return -1;
            }
            if (!s.has(left)) {
                cut = true;
                s.pos = s.n;
                return -1;
            }
        }
        --left;
        return s.u8();
    }
    // moves s.pos behind the chain's zero length; false when the data ends first
    bool finish() {
        if (cut) return false;
        if (closed) return true;
        s.pos += left;
        left = 0;
        closed = skip_chain(s);
        cut = !closed;
        return closed;
    }
};

// the LZW stream at s.pos -> out[0 .. total); s.pos ends behind the chain
inline int lzw_frame(Source& s, int min_code, uint8_t* out, int64_t total, Error& err) {
    uint16_t prefix[4096], length[4096];
    uint8_t suffix[4096], first[4096];
    const int clear = 1 << min_code, eoi = clear + 1;
    for (int i = 0; i < clear; ++i) {
        prefix[i] = 0;
        length[i] = 1;
        suffix[i] = first[i] = (uint8_t)i;
    }
    int next = clear + 2, width = min_code + 1, prev = -1;
    uint32_t acc = 0;
    int nbits = 0;
    int64_t npix = 0;
    Chain chain(s);
    while (npix < total) {
        const int64_t at = s.pos;
        while (nbits < width) {
            const int b = chain.next();
            if (b < 0) break;
            acc |= (uint32_t)b << nbits;
            nbits += 8;
        }
        if (nbits < width) break;                             // the chain ended
        const int code = (int)(acc & ((1u << width) - 1u));
        acc >>= width;
        nbits -= width;
        if (code == clear) {
            next = clear + 2;
            width = min_code + 1;
            prev = -1;
            continue;
        }
        if (code == eoi) break;
        if (prev < 0) {
            if (code > clear) {
                err = {at, "the first LZW code after a clear code is not a literal"};
                return E_ARG;
            }
            out[npix++] = (uint8_t)code;
            prev = code;
            if (next >= (1 << width)) ++width;                // (minimum code size 1 only: 4 entries fill 2 bits from the start)
            continue;
        }
        if (code > next || (code == next && next == 4096)) {
            err = {at, "an LZW code above the next free table entry"};
            return E_ARG;
        }
        if (next < 4096) {                                    // (a full table: the deferred clear, nothing is added)
            prefix[next] = (uint16_t)prev;
            suffix[next] = code < next ? first[code] : first[prev];
            first[next] = first[prev];
            length[next] = (uint16_t)(length[prev] + 1);
            ++next;
            if (next == (1 << width) && width < 12) ++width;
        }
        const int len = length[code];
        int c = code;
        for (int i = len - 1; i >= 0; --i) {
            if (npix + i < total) out[npix + i] = suffix[c];
            c = prefix[c];
        }
        npix += len;
        prev = code;
    }
    if (npix < total) {
        chain.finish();
        err = {s.pos, chain.cut ? "the data ends inside an image's sub-blocks" : "an image's LZW data ends before w * h pixels"};
        return E_ARG;
    }
    if (!chain.finish()) {
        err = {s.pos, "the data ends inside an image's sub-blocks"};
        return E_ARG;
    }
    return OK;
}

// rows of an interlaced frame in storage order -> display order
inline void deinterlace(const uint8_t* stored, int w, int h, uint8_t* out) {
    static const int START[4] = {0, 4, 2, 1}, STEP[4] = {8, 8, 4, 2};
    int r = 0;
    for (int p = 0; p < 4; ++p)
        for (int y = START[p]; y < h; y += STEP[p]) memcpy(out + (int64_t)y * w, stored + (int64_t)(r++) * w, (size_t)w);
}

// info[8]: W, H, frames F, colour tables P, raster bytes (sum of w * h), loop count (-1: no NETSCAPE extension), 1 if a global table
// exists, the version (87 / 89).  With frames == nullptr nothing is decoded (the probe); else frames[F][8], delays[F],
// palettes[P][256][4] and raster[0 .. raster_cap) are filled -- F and P are the probe's of the same bytes.
inline int walk(const uint8_t* data, int64_t n, int64_t* info, int32_t* frames, int32_t* delays, uint8_t* palettes, uint8_t* raster,
                int64_t raster_cap, Error& err) {
    const bool decode = frames != nullptr;
    Source s = {data, n, 0};
    const auto bad = [&](int64_t at, const char* what) {
        err = {at, what};
        return (int)E_ARG;
    };
    if (!s.has(6) || (memcmp(data, "GIF89a", 6) != 0 && memcmp(data, "GIF87a", 6) != 0)) return bad(0, "not a GIF (bad signature)");
    s.pos = 6;
    if (!s.has(7)) return bad(n, "the data ends inside the logical screen descriptor");
    const int W = s.u16(), H = s.u16(), packed = s.u8();
    s.pos += 2;                                               // background colour index, aspect ratio
    if (W == 0 || H == 0) return bad(6, "an empty canvas");
    int64_t F = 0, P = 0, total = 0, loop = -1;
    const bool global = (packed & 0x80) != 0;
    const auto table = [&](int flags) {                       // the colour table of 2 << (flags & 7) entries at s.pos -> row P
        const int size = 2 << (flags & 7);
        if (!s.has(3 * size)) return false;
        if (decode) {
            uint8_t* row = palettes + P * 1024;
            memset(row, 0, 1024);
            for (int i = 0; i < size; ++i) memcpy(row + 4 * i, data + s.pos + 3 * i, 3);
        }
        s.pos += 3 * size;
        ++P;
        return true;
    };
    if (global && !table(packed)) return bad(n, "the data ends inside the global colour table");
    int gce_delay = 0, gce_transparent = -1, gce_disposal = 0;
    std::vector<uint8_t> stored;
    for (;;) {
        if (!s.has(1)) {                                      // no trailer
            if (F == 0) return bad(n, "no frames");
            break;
        }
        const int64_t at = s.pos;
        const int block = s.u8();
        if (block == 0x3B) {
            if (F == 0) return bad(at, "no frames");
            break;
        }
        if (block == 0x21) {
            if (!s.has(1)) return bad(n, "the data ends inside an extension");
            const int label = s.u8();
            if (label == 0xF9 && s.has(1) && data[s.pos] >= 4 && s.has(1 + data[s.pos])) {
                const uint8_t* g = data + s.pos + 1;
                gce_disposal = (g[0] >> 2) & 7;
                if (gce_disposal > 3) gce_disposal = 0;
                gce_delay = g[1] | (g[2] << 8);
                gce_transparent = (g[0] & 1) ? g[3] : -1;
            } else if (label == 0xFF && s.has(1) && data[s.pos] == 11 && s.has(12 + 4) &&
                       (memcmp(data + s.pos + 1, "NETSCAPE2.0", 11) == 0 || memcmp(data + s.pos + 1, "ANIMEXTS1.0", 11) == 0)) {
                const uint8_t* a = data + s.pos + 12;
                if (a[0] >= 3 && a[1] == 1) loop = a[2] | (a[3] << 8);
            }
            if (!skip_chain(s)) return bad(s.pos, "the data ends inside an extension's sub-blocks");
            continue;
        }
        if (block != 0x2C) return bad(at, "an unknown block");
        if (!s.has(9)) return bad(n, "the data ends inside an image descriptor");
        const int x = s.u16(), y = s.u16(), w = s.u16(), h = s.u16(), flags = s.u8();
        if (w == 0 || h == 0) return bad(at, "an image of zero width or height");
        if (x + w > W || y + h > H) return bad(at, "an image that leaves the canvas");
        int64_t row = 0;
        if (flags & 0x80) {
            row = P;
            if (!table(flags)) return bad(n, "the data ends inside a local colour table");
        } else if (!global) {
            return bad(at, "an image with neither a local nor a global colour table");
        }
        if (!s.has(1)) return bad(n, "the data ends before an image's minimum code size");
        const int min_code = s.u8();
        if (min_code < 1 || min_code > 8) return bad(s.pos - 1, "an LZW minimum code size outside 1 .. 8");
        const int64_t pixels = (int64_t)w * h;
        if (total + pixels > MAX_RASTER) {
            err = {at, "the frames hold more than 2^31 - 1 pixels"};
            return E_CAP;
        }
        if (decode) {
            if (total + pixels > raster_cap) {
                err = {at, "the raster buffer is too small (gsdd_gif_probe gives the size)"};
                return E_CAP;
            }
            uint8_t* dst = raster + total;
            const bool interlaced = (flags & 0x40) != 0 && h > 1;
            if (interlaced) stored.resize((size_t)pixels);
            const int rc = lzw_frame(s, min_code, interlaced ? stored.data() : dst, pixels, err);
            if (rc != OK) return rc;
            if (interlaced) deinterlace(stored.data(), w, h, dst);
            int32_t* f = frames + F * 8;
            f[0] = x, f[1] = y, f[2] = w, f[3] = h;
            f[4] = (int32_t)total, f[5] = (int32_t)row, f[6] = gce_transparent, f[7] = gce_disposal;
            delays[F] = gce_delay;
        } else if (!skip_chain(s)) {
            return bad(s.pos, "the data ends inside an image's sub-blocks");
        }
        total += pixels;
        ++F;
        gce_delay = 0, gce_transparent = -1, gce_disposal = 0;
    }
    if (info) {
        info[0] = W, info[1] = H, info[2] = F, info[3] = P, info[4] = total, info[5] = loop, info[6] = global ? 1 : 0;
        info[7] = data[4] == '7' ? 87 : 89;
    }
    return OK;
}

}  // namespace gifr
}  // namespace gsdd
