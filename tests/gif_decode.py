"""A small GIF89a reader for the tests of gan_ode_amd.video_io: the textbook variable-width LZW decoder and a parser of the
blocks write_gif emits.  Written against the GIF89a specification, independent of the encoder in csrc/gif_lzw.h."""
import struct
from types import SimpleNamespace

import numpy as np


def lzw_decode(data, min_code_size):
    """A GIF code stream (the sub-blocks' payload, joined) -> namespace: data (uint8 array), clears (clear codes seen, the
    leading one included), codes (data codes since the last clear code), code_lengths (the indices every data code of the stream
    stands for, in order), eoi_width (the width the end code was read at).
    Raises ValueError on anything a conforming stream cannot hold."""
    data = bytes(data)
    clear, eoi = 1 << min_code_size, (1 << min_code_size) + 1
    table = [bytes([i]) for i in range(clear)] + [b"", b""]
    width, prev, acc, nbits, pos = min_code_size + 1, None, 0, 0, 0
    out, clears, codes, lengths = [], 0, 0, []
    while True:
        while nbits < width:
            if pos >= len(data):
                raise ValueError("the stream ends before the end-of-information code")
            acc |= data[pos] << nbits
            pos += 1
            nbits += 8
        code = acc & ((1 << width) - 1)
        acc >>= width
        nbits -= width
        if code == clear:
            del table[clear + 2:]
            width, prev, clears, codes = min_code_size + 1, None, clears + 1, 0
            continue
        if code == eoi:
            if pos != len(data):
                raise ValueError(f"{len(data) - pos} bytes behind the end-of-information code")
            return SimpleNamespace(data=np.frombuffer(b"".join(out), dtype=np.uint8), clears=clears, codes=codes,
                                   code_lengths=lengths, eoi_width=width)
        if clears == 0:
            raise ValueError("the stream does not open with a clear code")
        codes += 1
        if prev is None:
            if code >= clear:
                raise ValueError(f"code {code} straight behind a clear code")
            entry = table[code]
        else:
            if code < len(table):
                entry = table[code]
            elif code == len(table) and len(table) < 4096:
                entry = prev + prev[:1]
            else:
                raise ValueError(f"code {code} with a table of {len(table)}")
            if len(table) < 4096:
                table.append(prev + entry[:1])
        out.append(entry)
        lengths.append(len(entry))
        if len(table) == (1 << width) and width < 12:
            width += 1
        prev = entry


def _sub_blocks(buf, pos):
    """-> (payload, sizes of the sub-blocks, position behind the terminator)"""
    parts, sizes = [], []
    while True:
        n = buf[pos]
        pos += 1
        if n == 0:
            return b"".join(parts), sizes, pos
        parts.append(buf[pos:pos + n])
        if len(parts[-1]) != n:
            raise ValueError("a sub-block runs past the end of the file")
        sizes.append(n)
        pos += n


def read_gif(path):
    """-> namespace: version, width, height, palette (uint8 [k, 3], the global colour table), background, loop (None without a
    NETSCAPE2.0 block), frames (uint8 [T, H, W] indices), delays (hundredths of a second per frame), disposals,
    min_code_sizes, max_sub_block (the longest data sub-block), lzw (the decoders' namespaces per frame).  Only what write_gif
    emits is understood: full-screen, non-interlaced frames without local colour tables."""
    buf = open(path, "rb").read()
    g = SimpleNamespace(version=buf[:6], loop=None, delays=[], disposals=[], min_code_sizes=[], max_sub_block=0, lzw=[])
    g.width, g.height, packed, g.background, aspect = struct.unpack("<HHBBB", buf[6:13])
    pos = 13
    g.palette = None
    if packed & 0x80:
        k = 2 << (packed & 7)
        g.palette = np.frombuffer(buf[pos:pos + 3 * k], dtype=np.uint8).reshape(k, 3)
        pos += 3 * k
    frames, pending = [], None
    while True:
        tag = buf[pos]
        pos += 1
        if tag == 0x3B:
            if pos != len(buf):
                raise ValueError("bytes behind the trailer")
            break
        if tag == 0x21:
            label = buf[pos]
            pos += 1
            payload, sizes, pos = _sub_blocks(buf, pos)
            if label == 0xF9:
                if sizes != [4]:
                    raise ValueError("graphic control extension of the wrong size")
                flags, delay, _transparent = struct.unpack("<BHB", payload)
                pending = (delay, (flags >> 2) & 7)
            elif label == 0xFF and payload[:11] == b"NETSCAPE2.0":
                if sizes != [11, 3] or payload[11] != 1:
                    raise ValueError("malformed NETSCAPE2.0 block")
                g.loop = struct.unpack("<H", payload[12:14])[0]
            continue
        if tag != 0x2C:
            raise ValueError(f"unknown block {tag:#x} at {pos - 1}")
        left, top, w, h, flags = struct.unpack("<HHHHB", buf[pos:pos + 9])
        pos += 9
        if (left, top, w, h) != (0, 0, g.width, g.height) or flags != 0:
            raise ValueError("only full-screen frames without a local colour table are read")
        mcs = buf[pos]
        pos += 1
        payload, sizes, pos = _sub_blocks(buf, pos)
        d = lzw_decode(payload, mcs)
        if d.data.size != w * h:
            raise ValueError(f"a frame of {d.data.size} indices on a screen of {w} x {h}")
        frames.append(d.data.reshape(h, w))
        g.lzw.append(d)
        g.min_code_sizes.append(mcs)
        g.max_sub_block = max([g.max_sub_block] + sizes)
        g.delays.append(None if pending is None else pending[0])
        g.disposals.append(None if pending is None else pending[1])
        pending = None
    g.frames = np.stack(frames)
    return g
