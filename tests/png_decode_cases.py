"""The fixtures of the PNG decoder's tests (tests/golden/png_dec.{json,npz}, png_dec_512.npz: tools/make_golden_png.py) and the files the tests make
out of them: one per refusal of include/lsppng.h (container refusals by editing a fixture's chunks and re-sealing the CRCs; stream refusals by writing
the deflate stream bit by bit and sealing Adler-32 and CRCs around it), and the re-sealed single-byte changes.  Test infrastructure, shared by the CPU
and the GPU file."""
import functools
import hashlib
import json
import os
import struct
import zlib

import numpy as np

import png_decode_model as D
import png_writer as W
from conftest import GOLDEN

UNSUPPORTED, CORRUPT = D.UNSUPPORTED, D.CORRUPT


@functools.lru_cache(maxsize=None)
def fixtures():
    """(meta, {name: bytes}, {name: Pillow's pixels})"""
    with open(os.path.join(GOLDEN, "png_dec.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(GOLDEN, "png_dec.npz"))
    files = {k[:-4]: z[k].tobytes() for k in z.files if k.endswith(".png")}
    pixels = {k[:-3]: z[k] for k in z.files if k.endswith(".px")}
    return meta, files, pixels


def small_names():
    return [c["name"] for c in fixtures()[0]["cases"]]


@functools.lru_cache(maxsize=None)
def candidates():
    """[(name, bytes)] of the four 512 x 512 files, in the json's order"""
    z = np.load(os.path.join(GOLDEN, "png_dec_512.npz"))
    return [(c["name"], z[c["name"] + ".png"].tobytes()) for c in fixtures()[0]["candidates"]]


@functools.lru_cache(maxsize=None)
def candidate_pixels():
    """{name: uint8 [512, 512, 3]}: the model's pixels, which must hash to what Pillow returned when the fixtures were written"""
    out = {}
    for (name, data), c in zip(candidates(), fixtures()[0]["candidates"]):
        px = D.decode(data)
        assert hashlib.sha256(px.tobytes()).hexdigest() == c["pixels_sha256"], name
        out[name] = px
    return out


# ---- container edits -----------------------------------------------------------------------------------------------------------------------
def _edit(data, fn):
    """the file rebuilt from fn(list of [type, body]) with fresh CRCs"""
    return W.rebuild(fn([[c[0], c[1]] for c in W.chunks_of(data)]))


def _ihdr(data, **kw):
    def fn(chunks):
        w, h, d, ct, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
        v = dict(width=w, height=h, depth=d, color_type=ct, compression=comp, filter_method=flt, interlace=lace)
        v.update(kw)
        chunks[0][1] = struct.pack(">IIBBBBB", v["width"], v["height"], v["depth"], v["color_type"], v["compression"], v["filter_method"], v["interlace"])
        return chunks
    return _edit(data, fn)


def _insert(data, before_type, ctype, body=b""):
    def fn(chunks):
        k = next(i for i, c in enumerate(chunks) if c[0] == before_type)
        return chunks[:k] + [[ctype, body]] + chunks[k:]
    return _edit(data, fn)


def _drop(data, ctype):
    return _edit(data, lambda chunks: [c for c in chunks if c[0] != ctype])


def _body(data, ctype, body):
    def fn(chunks):
        for c in chunks:
            if c[0] == ctype:
                c[1] = body
        return chunks
    return _edit(data, fn)


def _zlib_header(data, cmf, flg):
    z = W.idat_of(data)
    return W.with_idat(data, bytes([cmf, flg]) + z[2:])


# ---- streams written bit by bit --------------------------------------------------------------------------------------------------------------
BASE_RAW = bytes([0, 1, 2, 3, 4, 1, 5, 6, 7, 8])              # a 4 x 2 grey file: filters None and Sub


def _grey(body, raw=BASE_RAW, adler=None, tail=b""):
    return W.png(4, 2, 8, 0, W.zlib_stream(body, raw, adler) + tail)


def _lits(raw):
    return [("lit", v) for v in raw]


def _stream_refusals():
    out = []

    def bits(*fields):
        w = W.BitWriter()
        for v, n in fields:
            w.bits(v, n)
        return w.done() + bytes(8)

    def fixed(tokens, extra=None):
        w = W.BitWriter()
        if extra is None:
            W.fixed_block(w, tokens)
        else:
            w.bits(1, 1)
            w.bits(1, 2)
            extra(w)
        return w.done()

    def dynamic(lit, dist, **kw):
        """the header of a dynamic block alone: these files are refused inside it"""
        w = W.BitWriter()
        W.dynamic_header(w, lit, dist, **kw)
        return w.done()

    lit_fixed, dist_fixed = W.canonical(W.FIXED_LIT), W.canonical(W.FIXED_DIST)
    out.append(("block type 3", _grey(bits((1, 1), (3, 2)))))
    w = W.BitWriter()
    W.stored_block(w, BASE_RAW, nlen=len(BASE_RAW))
    out.append(("a stored block whose LEN is not the complement of NLEN", _grey(w.done())))
    out.append(("HLIT above 286", _grey(bits((1, 1), (2, 2), (30, 5), (0, 5), (0, 4)))))
    out.append(("HDIST above 30", _grey(bits((1, 1), (2, 2), (0, 5), (30, 5), (0, 4)))))
    out.append(("a repeat code 16 with nothing before it", _grey(dynamic([8] * 257, [1, 1], raw_cl_symbols=[(16, 0)] + [(8, None)] * 10) + bytes(8))))
    out.append(("a repeat that runs past HLIT + HDIST", _grey(dynamic([8] * 257, [1], raw_cl_symbols=[(8, None)] * 256 + [(18, 127)]) + bytes(8))))
    out.append(("no code for symbol 256", _grey(dynamic([8] * 256 + [0], [1, 1]) + bytes(8))))
    out.append(("an over-subscribed code-length set", _grey(dynamic([1, 1] + [0] * 254 + [1], [1, 1]) + bytes(8))))
    out.append(("an incomplete code-length set", _grey(dynamic([2, 2] + [0] * 254 + [2], [1, 1]) + bytes(8))))
    out.append(("an incomplete distance code of two bits", _grey(dynamic(W.FLAT_LIT, [2, 2, 2]) + bytes(8))))
    cl = [0] * 19
    cl[8] = 1
    out.append(("an incomplete code-length code", _grey(dynamic([8] * 257, [8], cl_lengths=cl) + bytes(8))))
    # a distance code of a single one-bit code is admitted; the OTHER bit pattern is in no code
    w = W.BitWriter()
    W.dynamic_header(w, W.FLAT_LIT, [1])
    for v in BASE_RAW[:6]:
        w.code(*W.canonical(W.FLAT_LIT)[v])
    w.code(*W.canonical(W.FLAT_LIT)[257])                      # length 3
    w.code(1, 1)                                               # the distance code is '0'
    out.append(("a bit pattern that is in no code", _grey(w.done() + bytes(8))))

    def len286(w):
        for v in BASE_RAW[:4]:
            w.code(*lit_fixed[v])
        w.code(*lit_fixed[286])
    out.append(("length symbol 286", _grey(fixed(None, len286) + bytes(8))))

    def dist30(w):
        for v in BASE_RAW[:4]:
            w.code(*lit_fixed[v])
        w.code(*lit_fixed[257])
        w.code(*dist_fixed[30])
    out.append(("distance symbol 30", _grey(fixed(None, dist30) + bytes(8))))
    out.append(("a distance that reaches before the first output byte", _grey(fixed([("lit", 0), ("match", 3, 2)] + _lits(BASE_RAW[4:])))))
    out.append(("output that would pass H x (1 + rowbytes) bytes", _grey(fixed(_lits(BASE_RAW + b"\x09")))))
    out.append(("a final block that ends short", _grey(fixed(_lits(BASE_RAW[:-1])), raw=BASE_RAW[:-1])))
    body = fixed(_lits(BASE_RAW))
    out.append(("input that ends inside the stream", W.png(4, 2, 8, 0, W.ZLIB_HEADER + body[:len(body) // 2])))
    out.append(("input that ends inside the Adler-32", W.png(4, 2, 8, 0, W.zlib_stream(body, BASE_RAW)[:-2])))
    out.append(("an Adler-32 that does not match", _grey(body, adler=struct.pack(">I", zlib.adler32(BASE_RAW) ^ 1))))
    out.append(("bytes left in the IDAT data after the Adler-32", _grey(body, tail=b"\x00")))
    bad = bytes([0, 1, 2, 3, 4, 5, 5, 6, 7, 8])
    out.append(("a filter byte above 4", _grey(fixed(_lits(bad)), raw=bad)))
    raw = bytes([0, 0, 1, 2, 0, 2, 3, 0])                      # 3 x 2 indices at depth 8, three PLTE entries: index 3 is past them
    out.append(("a palette index at or past the PLTE entry count", W.png(3, 2, 8, 3, W.zlib_stream(fixed(_lits(raw)), raw), palette=bytes(range(9)))))
    raw = bytes([0, 0x01, 0x20, 0, 0x13, 0x00])                # 3 x 2 indices at depth 4 (the last nibble of a row is padding), three entries
    out.append(("a palette index past the PLTE entries at depth 4", W.png(3, 2, 4, 3, W.zlib_stream(fixed(_lits(raw)), raw), palette=bytes(range(9)))))
    return [(what, data, CORRUPT) for what, data in out]


@functools.lru_cache(maxsize=None)
def stream_refusals():
    """[(what, file, CORRUPT)]: one per line of the header's stream-level list; these run on the device too"""
    return _stream_refusals()


@functools.lru_cache(maxsize=None)
def admitted():
    """[(what, file)]: files that stand next to a refusal and are decoded: the padding nibble of a depth-4 row may hold any value"""
    w = W.BitWriter()
    raw = bytes([0, 0x01, 0x2F, 0, 0x12, 0x0F])
    W.fixed_block(w, _lits(raw))
    return [("a depth-4 row whose padding nibble is past the PLTE entries", W.png(3, 2, 4, 3, W.zlib_stream(w.done(), raw), palette=bytes(range(9))))]


@functools.lru_cache(maxsize=None)
def refusals():
    """[(what, file, status)]: one per line of the UNSUPPORTED and CORRUPT lists of include/lsppng.h"""
    _, files, _ = fixtures()
    rgb, pal, anc = files["rgb_31x17_l6"], files["p4_3x11"], files["rgb_12x10_ancillary"]
    out = [("Adam7 interlace", _ihdr(rgb, interlace=1), UNSUPPORTED),
           ("bit depth 16", _ihdr(rgb, depth=16), UNSUPPORTED),
           ("bit depth 16, grey + alpha", _ihdr(files["ga_21x67"], depth=16), UNSUPPORTED),
           ("grey at depth 1", _ihdr(files["grey_20x20"], depth=1), UNSUPPORTED),
           ("grey at depth 2", _ihdr(files["grey_20x20"], depth=2), UNSUPPORTED),
           ("grey at depth 4", _ihdr(files["grey_20x20"], depth=4), UNSUPPORTED),
           ("a width above max_side", _ihdr(rgb, width=8193), UNSUPPORTED),
           ("a height above max_side", _ihdr(rgb, height=8193), UNSUPPORTED),
           ("APNG: acTL", _insert(rgb, b"IDAT", b"acTL", struct.pack(">II", 1, 0)), UNSUPPORTED),
           ("APNG: fcTL", _insert(rgb, b"IDAT", b"fcTL", bytes(26)), UNSUPPORTED),
           ("APNG: fdAT", _insert(rgb, b"IEND", b"fdAT", bytes(8)), UNSUPPORTED),
           ("an unknown critical chunk", _insert(rgb, b"IDAT", b"CrIT", b"?"), UNSUPPORTED)]
    c = []
    c.append(("a wrong signature", b"\x88" + rgb[1:]))
    c.append(("a chunk that runs past the file", rgb[:-12] + struct.pack(">I", 4) + rgb[-8:]))
    at = W.chunks_of(rgb)[1][2]
    c.append(("a wrong CRC on IDAT", rgb[:at + 8] + bytes([rgb[at + 8] ^ 1]) + rgb[at + 9:]))
    at = next(ch[2] for ch in W.chunks_of(anc) if ch[0] == b"tEXt")
    c.append(("a wrong CRC on tEXt", anc[:at + 10] + bytes([anc[at + 10] ^ 0x20]) + anc[at + 11:]))
    c.append(("a chunk type with a non-letter byte", _edit(anc, lambda ch: [[b"tE1t" if t == b"tEXt" else t, b] for t, b in ch])))
    c.append(("IHDR not first", _edit(rgb, lambda ch: [[b"tEXt", b"a\0b"]] + ch)))
    c.append(("IHDR not 13 bytes", _edit(rgb, lambda ch: [[ch[0][0], ch[0][1] + b"\0"]] + ch[1:])))
    c.append(("IHDR repeated", _edit(rgb, lambda ch: [ch[0], ch[0]] + ch[1:])))
    c.append(("zero width", _ihdr(rgb, width=0)))
    c.append(("zero height", _ihdr(rgb, height=0)))
    c.append(("compression method not 0", _ihdr(rgb, compression=1)))
    c.append(("filter method not 0", _ihdr(rgb, filter_method=1)))
    c.append(("interlace method 2", _ihdr(rgb, interlace=2)))
    c.append(("an illegal colour type / bit depth pair: RGB at depth 4", _ihdr(rgb, depth=4)))
    c.append(("an illegal colour type", _ihdr(rgb, color_type=5)))
    c.append(("an illegal depth: palette at 16", _ihdr(pal, depth=16)))
    c.append(("an illegal depth: 3", _ihdr(rgb, depth=3)))
    c.append(("PLTE missing", _drop(pal, b"PLTE")))
    plte = next(ch[1] for ch in W.chunks_of(pal) if ch[0] == b"PLTE")
    c.append(("PLTE after IDAT", _insert(_drop(pal, b"PLTE"), b"IEND", b"PLTE", plte)))
    c.append(("PLTE repeated", _insert(pal, b"IDAT", b"PLTE", plte)))
    c.append(("PLTE of a length not divisible by 3", _body(pal, b"PLTE", plte + b"\0")))
    c.append(("PLTE empty", _body(pal, b"PLTE", b"")))
    c.append(("PLTE with more than 2^depth entries", _body(pal, b"PLTE", bytes(51))))
    z = W.idat_of(rgb)
    c.append(("IDAT chunks not consecutive", _edit(rgb, lambda ch: [ch[0], [b"IDAT", z[:20]], [b"tEXt", b"a\0b"], [b"IDAT", z[20:]], ch[-1]])))
    c.append(("no IDAT", _drop(rgb, b"IDAT")))
    c.append(("IEND missing", _drop(rgb, b"IEND")))
    c.append(("IEND not empty", _body(rgb, b"IEND", b"x")))
    c.append(("bytes after IEND", rgb + b"\0"))
    c.append(("a zlib header whose CM is not 8", _zlib_header(rgb, 0x79, next(f for f in range(32) if (0x7900 + f) % 31 == 0))))
    c.append(("a zlib header whose CINFO is 8", _zlib_header(rgb, 0x88, next(f for f in range(0, 32) if (0x8800 + f) % 31 == 0))))
    c.append(("a zlib header whose check bits are wrong", _zlib_header(rgb, 0x78, 0x9D)))
    c.append(("a zlib header with FDICT", _zlib_header(rgb, 0x78, next(f for f in range(32, 64) if (0x7800 + f) % 31 == 0))))
    c.append(("IDAT data of one byte", W.with_idat(rgb, b"\x78")))
    out += [(what, data, CORRUPT) for what, data in c]
    return out + list(stream_refusals())


# ---- re-sealed changes: one byte of the deflate body flipped, Adler-32 and CRCs made right again -----------------------------------------------
def resealed(data, rng):
    z = W.idat_of(data)
    body = bytearray(z[2:-4])
    body[int(rng.integers(len(body)))] ^= int(rng.integers(1, 256))
    adler = z[-4:]
    try:
        d = zlib.decompressobj(-15)
        raw = d.decompress(bytes(body)) + d.flush()
        if d.eof:
            adler = struct.pack(">I", zlib.adler32(raw))
    except zlib.error:
        pass
    return W.with_idat(data, z[:2] + bytes(body) + adler)
