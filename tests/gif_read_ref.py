"""The GIF import restated in numpy (csrc/gif_read_host.hpp, csrc/gif_read.hip) -- this restatement is the definition -- and a small
GIF builder for the tests that can write what the library's own writer cannot: sub-rectangles, transparent indices, disposals,
interlace, local and global tables of 2 .. 256 entries, minimum code sizes 1 .. 8, chosen sub-block lengths, a clear code at 4096
table entries or deferred for ever, a missing trailer.

File walk: header, logical screen descriptor, global colour table; then 0x21 extensions (0xF9: disposal / transparent index / delay of
the next image; 0xFF "NETSCAPE2.0": loop count; others skipped), 0x2C images, the trailer 0x3B or the end of the data.

LZW (decoder and builder share one convention, the one of the library's writer and of giflib): `free` is the next free table entry;
every code except a clear code that follows at least one other code since the last clear code adds an entry; the width grows by one
bit when `free` reaches 1 << width (at most 12) -- and, with a minimum code size of 1, once more right behind the first code after a
clear code, where free = 4 = 1 << 2 already; with 4096 entries nothing is added and the width stays 12."""
import numpy as np


class GifError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------- decoder
def _chain(data, pos):
    """the bytes of the sub-block chain at pos -> (payload, position behind the zero length); GifError when the data ends first"""
    out = bytearray()
    while True:
        if pos >= len(data):
            raise GifError("sub-block chain cut off")
        n = data[pos]
        pos += 1
        if n == 0:
            return bytes(out), pos
        if pos + n > len(data):
            raise GifError("sub-block chain cut off")
        out += data[pos:pos + n]
        pos += n


def lzw_decode(payload, min_code, total):
    """the first `total` pixels of an LZW stream (without its sub-block framing)"""
    clear, eoi = 1 << min_code, (1 << min_code) + 1
    table = [bytes([i]) for i in range(clear)] + [b"", b""]
    width, prev = min_code + 1, None
    out = bytearray()
    acc = nbits = pos = 0
    while len(out) < total:
        while nbits < width and pos < len(payload):
            acc |= payload[pos] << nbits
            nbits += 8
            pos += 1
        if nbits < width:
            break
        code = acc & ((1 << width) - 1)
        acc >>= width
        nbits -= width
        if code == clear:
            del table[clear + 2:]
            width, prev = min_code + 1, None
            continue
        if code == eoi:
            break
        if prev is None:
            if code > clear:
                raise GifError("first code after a clear code is not a literal")
            out += table[code]
            prev = code
            if len(table) >= (1 << width) and width < 12:          # (minimum code size 1 only)
                width += 1
            continue
        if code > len(table) or (code == len(table) == 4096):
            raise GifError("code above the next free entry")
        entry = table[code] if code < len(table) else table[prev] + table[prev][:1]
        if len(table) < 4096:
            table.append(table[prev] + entry[:1])
            if len(table) == (1 << width) and width < 12:
                width += 1
        out += entry
        prev = code
    if len(out) < total:
        raise GifError("data ends before w * h pixels")
    return np.frombuffer(bytes(out[:total]), dtype=np.uint8)


def interlace_rows(h):
    """storage order of an interlaced frame: the display rows in the order they are stored"""
    return [y for start, step in ((0, 8), (4, 8), (2, 4), (1, 2)) for y in range(start, h, step)]


def decode(data):
    """-> dict(width, height, loop, global_table, frames (F, 8) int32, delays (F,) int32, palettes (P, 256, 4) uint8, raster uint8)"""
    data = bytes(data)
    if len(data) < 6 or data[:6] not in (b"GIF87a", b"GIF89a"):
        raise GifError("bad signature")
    if len(data) < 13:
        raise GifError("truncated")
    W, H = data[6] | data[7] << 8, data[8] | data[9] << 8
    if W == 0 or H == 0:
        raise GifError("empty canvas")
    palettes, frames, delays, rasters = [], [], [], []
    pos = 13

    def table(flags):
        nonlocal pos
        n = 2 << (flags & 7)
        if pos + 3 * n > len(data):
            raise GifError("truncated colour table")
        row = np.zeros((256, 4), dtype=np.uint8)
        row[:n, :3] = np.frombuffer(data[pos:pos + 3 * n], dtype=np.uint8).reshape(n, 3)
        palettes.append(row)
        pos += 3 * n

    has_global = bool(data[10] & 0x80)
    if has_global:
        table(data[10])
    loop, total = -1, 0
    delay, transparent, disposal = 0, -1, 0
    while True:
        if pos >= len(data):
            break
        block = data[pos]
        pos += 1
        if block == 0x3B:
            break
        if block == 0x21:
            if pos >= len(data):
                raise GifError("truncated extension")
            label = data[pos]
            pos += 1
            start = pos
            _, pos = _chain(data, pos)
            first = data[start + 1:start + 1 + data[start]]
            if label == 0xF9 and len(first) >= 4:
                disposal = (first[0] >> 2) & 7
                disposal = 0 if disposal > 3 else disposal
                delay = first[1] | first[2] << 8
                transparent = first[3] if first[0] & 1 else -1
            elif label == 0xFF and first in (b"NETSCAPE2.0", b"ANIMEXTS1.0"):
                second = data[start + 12:start + 16]
                if len(second) == 4 and second[0] >= 3 and second[1] == 1:
                    loop = second[2] | second[3] << 8
            continue
        if block != 0x2C:
            raise GifError("unknown block")
        if pos + 9 > len(data):
            raise GifError("truncated image descriptor")
        x, y, w, h = (data[pos + 2 * i] | data[pos + 2 * i + 1] << 8 for i in range(4))
        flags = data[pos + 8]
        pos += 9
        if w == 0 or h == 0 or x + w > W or y + h > H:
            raise GifError("bad rectangle")
        row = 0
        if flags & 0x80:
            row = len(palettes)
            table(flags)
        elif not has_global:
            raise GifError("no colour table")
        if pos >= len(data):
            raise GifError("truncated")
        min_code = data[pos]
        pos += 1
        if not 1 <= min_code <= 8:
            raise GifError("bad minimum code size")
        payload, pos = _chain(data, pos)
        px = lzw_decode(payload, min_code, w * h).reshape(h, w)
        if flags & 0x40:
            shown = np.empty_like(px)
            shown[interlace_rows(h)] = px
            px = shown
        frames.append([x, y, w, h, total, row, transparent, disposal])
        delays.append(delay)
        rasters.append(px.reshape(-1))
        total += w * h
        delay, transparent, disposal = 0, -1, 0
    if not frames:
        raise GifError("no frames")
    return dict(width=W, height=H, loop=loop, global_table=int(has_global), frames=np.array(frames, dtype=np.int32),
                delays=np.array(delays, dtype=np.int32), palettes=np.stack(palettes), raster=np.concatenate(rasters))


# ---------------------------------------------------------------------------------------------- compositor
def compose(raster, frames, palettes, W, H, select, matte=(0, 0, 0)):
    """-> (len(select), H, W, 3) uint8.  Per pixel, from the matte: before frame f > 0 the disposal of frame f-1 inside ITS rectangle
    (2: the matte; 3: the value saved before f-1 was drawn; 0, 1: nothing); a frame with disposal 3 saves the pixel first; inside
    f's rectangle an index other than the transparent one sets palettes[row][index]; then every slot k with select[k] == f is written."""
    canvas = np.empty((H, W, 3), dtype=np.uint8)
    canvas[:] = np.array(matte, dtype=np.uint8)
    saved = canvas.copy()
    out = np.zeros((len(select), H, W, 3), dtype=np.uint8)
    for f in range(int(select[-1]) + 1):
        if f > 0:
            x, y, w, h, _, _, _, disposal = (int(v) for v in frames[f - 1])
            if disposal == 2:
                canvas[y:y + h, x:x + w] = np.array(matte, dtype=np.uint8)
            elif disposal == 3:
                canvas[y:y + h, x:x + w] = saved[y:y + h, x:x + w]
        x, y, w, h, off, row, transparent, disposal = (int(v) for v in frames[f])
        if disposal == 3:
            saved = canvas.copy()
        idx = np.asarray(raster[off:off + w * h]).reshape(h, w)
        rgb = palettes[row][idx.astype(np.int64), :3]
        region = canvas[y:y + h, x:x + w]
        canvas[y:y + h, x:x + w] = np.where((idx != transparent)[..., None], rgb, region)
        for k, s in enumerate(select):
            if int(s) == f:
                out[k] = canvas
    return out


# ---------------------------------------------------------------------------------------------- builder
def lzw_encode(px, min_code, clear_mode="full", stats=None):
    """pixels -> the LZW stream (no sub-block framing).  clear_mode "full": a clear code whenever the table holds 4096 entries (the
    library's writer); "deferred": never again -- the table stays full and codes stay 12 bits.  stats (a dict): receives the clear
    codes written and the codes written while the table was full."""
    clear, eoi = 1 << min_code, (1 << min_code) + 1
    out = bytearray()
    state = dict(acc=0, nbits=0, width=min_code + 1)

    def emit(code):
        state["acc"] |= code << state["nbits"]
        state["nbits"] += state["width"]
        while state["nbits"] >= 8:
            out.append(state["acc"] & 255)
            state["acc"] >>= 8
            state["nbits"] -= 8

    def count():                                                   # the writer's count runs one ahead of the reader's free entry
        nonlocal nxt
        nxt += 1
        if nxt > (1 << state["width"]) and state["width"] < 12:
            state["width"] += 1

    table, nxt = {}, clear + 2
    emit(clear)
    clears = at_full = 0
    px = [int(v) for v in px]
    prefix = px[0]
    for c in px[1:]:
        key = (prefix, c)
        if key in table:
            prefix = table[key]
            continue
        emit(prefix)
        if nxt < 4096:
            table[key] = nxt
            count()
        else:
            at_full += 1
        if nxt == 4096 and clear_mode == "full":
            emit(clear)
            clears += 1
            table, nxt = {}, clear + 2
            state["width"] = min_code + 1
        prefix = c
    emit(prefix)
    if nxt < 4096:
        count()
    emit(eoi)
    if state["nbits"]:
        out.append(state["acc"] & 255)
    if stats is not None:
        stats.update(clears=1 + clears, codes_at_full_table=at_full)
    return bytes(out)


def sub_blocks(payload, lengths=255):
    """frame a payload in sub-blocks: `lengths` an int or a cycle of ints in 1 .. 255"""
    cycle = [lengths] if isinstance(lengths, int) else list(lengths)
    out, pos, i = bytearray(), 0, 0
    while pos < len(payload):
        n = min(cycle[i % len(cycle)], len(payload) - pos)
        out.append(n)
        out += payload[pos:pos + n]
        pos += n
        i += 1
    out.append(0)
    return bytes(out)


def _bits(n):
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def _table(pal):
    pal = np.asarray(pal, dtype=np.uint8).reshape(-1, 3)
    bits = _bits(len(pal))
    full = np.zeros((1 << bits, 3), dtype=np.uint8)
    full[:len(pal)] = pal
    return bits, full.tobytes()


def _u16(v):
    return bytes([v & 255, (v >> 8) & 255])


def build_gif(W, H, frames, global_palette=None, loop=None, trailer=True, version=b"89a"):
    """frames: dicts with indices (h, w) uint8 and optionally x, y (0), palette (a local table, (n, 3)), transparent (an index),
    disposal (0 .. 7), delay (centiseconds) -- a graphic control extension is written when any of the last three is given --,
    interlace (False), min_code (the table's bits, at least 2), sub_block (255), clear ("full" / "deferred")."""
    out = bytearray(b"GIF" + version + _u16(W) + _u16(H))
    if global_palette is not None:
        bits, raw = _table(global_palette)
        out += bytes([0x80 | 0x70 | (bits - 1), 0, 0]) + raw
        gbits = bits
    else:
        out += bytes([0x70, 0, 0])
        gbits = None
    if loop is not None:
        out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + _u16(loop) + b"\x00"
    for fr in frames:
        idx = np.asarray(fr["indices"], dtype=np.uint8)
        h, w = idx.shape
        if any(k in fr for k in ("transparent", "disposal", "delay")):
            t = fr.get("transparent")
            out += bytes([0x21, 0xF9, 4, (fr.get("disposal", 0) << 2) | (0 if t is None else 1)]) + _u16(fr.get("delay", 0))
            out += bytes([0 if t is None else t, 0])
        out += b"\x2C" + _u16(fr.get("x", 0)) + _u16(fr.get("y", 0)) + _u16(w) + _u16(h)
        flags = 0x40 if fr.get("interlace") else 0
        if fr.get("palette") is not None:
            bits, raw = _table(fr["palette"])
            out += bytes([flags | 0x80 | (bits - 1)]) + raw
        else:
            bits, raw = gbits, b""
            out += bytes([flags])
        min_code = fr.get("min_code", max(2, bits if bits is not None else 8))
        stored = idx[interlace_rows(h)] if fr.get("interlace") else idx
        out.append(min_code)
        out += sub_blocks(lzw_encode(stored.reshape(-1), min_code, fr.get("clear", "full")), fr.get("sub_block", 255))
    if trailer:
        out.append(0x3B)
    return bytes(out)
