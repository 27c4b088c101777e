"""The PNG decoder of include/lsppng.h restated in Python, independently of the library: its own chunk walker, its own inflate (not ``zlib``, so that
it states every refusal of the stream), the unfilter of the PNG specification and the pixel fetch.  The second oracle of the tests beside Pillow:
``parse`` / ``inflate`` / ``unfilter`` / ``pixels`` are the planner and the three launches, ``decode`` all of them, ``status_of`` the status word."""
import binascii

import numpy as np

UNSUPPORTED, CORRUPT = 1, 2
SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_SIDE = 8192


class Refused(Exception):
    def __init__(self, status, why=""):
        super().__init__("%s (%d)" % (why, status))
        self.status = status


def _corrupt(why):
    return Refused(CORRUPT, why)


# ---- the container -----------------------------------------------------------------------------------------------------------------------
def parse(data, max_side=MAX_SIDE):
    """the chunk walk: a dict of the geometry, the palette and the concatenated IDAT payload; raises Refused.  A CORRUPT container is CORRUPT
    whatever else it holds; an UNSUPPORTED file's zlib header is not looked at."""
    data = bytes(data)
    n = len(data)
    if data[:8] != SIGNATURE:
        raise _corrupt("signature")
    at, f, first = 8, {}, True
    seen_plte = seen_idat = idat_done = seen_iend = unsupported = False
    idat = []
    while at < n:
        if n - at < 12:
            raise _corrupt("a chunk runs past the file")
        length = int.from_bytes(data[at:at + 4], "big")
        if length > n - at - 12:
            raise _corrupt("a chunk runs past the file")
        ctype, body = data[at + 4:at + 8], data[at + 8:at + 8 + length]
        if not all(65 <= c <= 90 or 97 <= c <= 122 for c in ctype):
            raise _corrupt("chunk type")
        if binascii.crc32(ctype + body) != int.from_bytes(data[at + 8 + length:at + 12 + length], "big"):
            raise _corrupt("CRC of %r" % ctype)
        if first != (ctype == b"IHDR"):
            raise _corrupt("IHDR not first, or repeated")
        if seen_idat and ctype != b"IDAT":
            idat_done = True
        if first:
            if length != 13:
                raise _corrupt("IHDR length")
            w, h = int.from_bytes(body[:4], "big"), int.from_bytes(body[4:8], "big")
            d, ct, comp, flt, lace = body[8:13]
            if w == 0 or h == 0 or w >> 31 or h >> 31 or comp or flt or lace > 1:
                raise _corrupt("IHDR values")
            if not (d in (1, 2, 4, 8, 16) and (ct == 0 or (ct == 3 and d <= 8) or (ct in (2, 4, 6) and d >= 8))):
                raise _corrupt("colour type / bit depth")
            ch = {0: 1, 3: 1, 4: 2, 2: 3, 6: 4}[ct]
            unsupported = lace == 1 or d == 16 or (ct == 0 and d < 8) or w > max_side or h > max_side
            f = {"width": w, "height": h, "depth": d, "color_type": ct, "channels": ch, "ncomp": 1 if ct in (0, 4) else 3,
                 "bpp": max(1, ch * d // 8), "rowbytes": (w * ch * d + 7) // 8, "palette": None}
            f["raw_bytes"] = h * (1 + f["rowbytes"])
        elif ctype == b"PLTE":
            if f["color_type"] == 3:
                if seen_plte or seen_idat or length % 3 or length == 0 or length // 3 > 1 << f["depth"]:
                    raise _corrupt("PLTE")
                seen_plte = True
                f["palette"] = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif ctype == b"IDAT":
            if idat_done or (f["color_type"] == 3 and not seen_plte):
                raise _corrupt("IDAT out of place")
            seen_idat = True
            idat.append(body)
        elif ctype == b"IEND":
            if length:
                raise _corrupt("IEND not empty")
            seen_iend = True
            at += 12
            break
        elif ctype in (b"acTL", b"fcTL", b"fdAT") or not ctype[0] & 0x20:
            unsupported = True
        first = False
        at += 12 + length
    if not seen_iend or at != n or not seen_idat:
        raise _corrupt("IEND missing, bytes after it, or no IDAT")
    if unsupported:
        raise Refused(UNSUPPORTED, "outside what is decoded")
    z = b"".join(idat)
    if len(z) < 2 or z[0] & 15 != 8 or z[0] >> 4 > 7 or (z[0] << 8 | z[1]) % 31 or z[1] & 32:
        raise _corrupt("zlib header")
    f["idat"] = z
    return f


# ---- inflate -----------------------------------------------------------------------------------------------------------------------------
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LITLEN, DIST, LENGTHS = "literal/length", "distance", "code length"


def _code(lengths, kind):
    """{(length, code): symbol} of a canonical code; refuses an over-subscribed set and an incomplete one, except a literal/length or distance code
    that is a single code of one bit, and a distance code without any code"""
    count = [0] * 16
    for v in lengths:
        count[v] += 1
    left = 1
    for k in range(1, 16):
        left = 2 * left - count[k]
        if left < 0:
            raise _corrupt("over-subscribed %s code" % kind)
    if left > 0:
        single = count[1] == 1 and count[0] == len(lengths) - 1
        empty = count[0] == len(lengths)
        if kind == LENGTHS or not (single or (empty and kind == DIST)):
            raise _corrupt("incomplete %s code" % kind)
    nxt, code = [0] * 16, 0
    for k in range(1, 16):
        code = (code + (count[k - 1] if k > 1 else 0)) << 1
        nxt[k] = code
    table = {}
    for s, v in enumerate(lengths):
        if v:
            table[(v, nxt[v])] = s
            nxt[v] += 1
    return table


class _Bits:
    def __init__(self, z, at):
        self.z, self.at, self.buf, self.cnt = z, at, 0, 0

    def take(self, n):
        while self.cnt < n:
            if self.at >= len(self.z):
                raise _corrupt("the input ends inside the stream")
            self.buf |= self.z[self.at] << self.cnt
            self.cnt += 8
            self.at += 1
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 16):
            code = code << 1 | self.take(1)
            s = table.get((length, code))
            if s is not None:
                return s
        raise _corrupt("a bit pattern that is in no code")


_FIXED = None


def inflate(z, expect):
    """the zlib stream z (header checked by parse) to exactly ``expect`` bytes, Adler-32 checked, nothing left over; raises Refused(CORRUPT)"""
    global _FIXED
    br, out = _Bits(z, 2), bytearray()
    while True:
        final, kind = br.take(1), br.take(2)
        if kind == 3:
            raise _corrupt("block type 3")
        if kind == 0:
            br.take(br.cnt & 7)
            length, nlength = br.take(16), br.take(16)
            if length ^ 0xFFFF != nlength:
                raise _corrupt("stored LEN / NLEN")
            br.at -= br.cnt >> 3
            br.buf = br.cnt = 0
            if len(out) + length > expect:
                raise _corrupt("output past the expected size")
            if br.at + length > len(z):
                raise _corrupt("the input ends inside the stream")
            out += z[br.at:br.at + length]
            br.at += length
        else:
            if kind == 1:
                if _FIXED is None:
                    _FIXED = (_code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, LITLEN), _code([5] * 32, DIST))
                lit, dist = _FIXED
            else:
                nlen, ndist, ncode = br.take(5) + 257, br.take(5) + 1, br.take(4) + 4
                if nlen > 286 or ndist > 30:
                    raise _corrupt("HLIT / HDIST")
                cl = [0] * 19
                for k in range(ncode):
                    cl[_ORDER[k]] = br.take(3)
                clcode, lengths = _code(cl, LENGTHS), []
                while len(lengths) < nlen + ndist:
                    s = br.symbol(clcode)
                    if s < 16:
                        lengths.append(s)
                        continue
                    if s == 16:
                        if not lengths:
                            raise _corrupt("repeat with nothing before it")
                        value, rep = lengths[-1], 3 + br.take(2)
                    elif s == 17:
                        value, rep = 0, 3 + br.take(3)
                    else:
                        value, rep = 0, 11 + br.take(7)
                    if len(lengths) + rep > nlen + ndist:
                        raise _corrupt("a repeat past HLIT + HDIST")
                    lengths += [value] * rep
                if lengths[256] == 0:
                    raise _corrupt("no code for symbol 256")
                lit, dist = _code(lengths[:nlen], LITLEN), _code(lengths[nlen:], DIST)
            while True:
                s = br.symbol(lit)
                if s < 256:
                    if len(out) >= expect:
                        raise _corrupt("output past the expected size")
                    out.append(s)
                elif s == 256:
                    break
                else:
                    s -= 257
                    if s >= 29:
                        raise _corrupt("length symbol 286 / 287")
                    length = _LBASE[s] + br.take(_LEXT[s])
                    ds = br.symbol(dist)
                    if ds >= 30:
                        raise _corrupt("distance symbol 30 / 31")
                    d = _DBASE[ds] + br.take(_DEXT[ds])
                    if d > len(out):
                        raise _corrupt("a distance before the first output byte")
                    if len(out) + length > expect:
                        raise _corrupt("output past the expected size")
                    seg = out[-d:]
                    out += (seg * (length // d + 1))[:length] if d < length else seg[:length]
        if final:
            break
    if len(out) != expect:
        raise _corrupt("the final block ends short of the expected size")
    br.take(br.cnt & 7)
    want = 0
    for _ in range(4):
        want = want << 8 | br.take(8)
    a = b = 0
    a, b = 1, 0
    view = np.frombuffer(bytes(out), np.uint8).astype(np.uint64)
    for k in range(0, len(view), 4096):                        # sums of 4096 bytes stay far below 2^64
        part = view[k:k + 4096]
        m = len(part)
        b = (b + m * a + int((part * np.arange(m, 0, -1, dtype=np.uint64)).sum())) % 65521
        a = (a + int(part.sum())) % 65521
    if want != (b << 16 | a):
        raise _corrupt("Adler-32")
    if br.cnt or br.at != len(z):
        raise _corrupt("bytes after the Adler-32")
    return bytes(out)


# ---- unfilter and pixels -------------------------------------------------------------------------------------------------------------------
def unfilter(f, raw):
    """the PNG specification's reconstruction over all rows at once, as a wavefront: byte x of row y at step x + y (its three neighbours belong to
    earlier steps).  uint8 [H, rowbytes]; raises Refused(CORRUPT) on a filter byte above 4."""
    h, rb, bpp = f["height"], f["rowbytes"], f["bpp"]
    lines = np.frombuffer(raw, np.uint8).reshape(h, 1 + rb)
    ft = lines[:, 0].astype(np.int64)
    if ft.max() > 4:
        raise _corrupt("a filter byte above 4")
    x = lines[:, 1:].astype(np.int64)
    r = np.zeros((h + 1, rb + bpp), np.int64)                  # a row of zeros above, bpp zeros to the left
    rows = np.arange(h)
    for t in range(rb + h - 1):
        ys = rows[max(0, t - rb + 1):min(h - 1, t) + 1]
        xs = t - ys
        a, b, c = r[ys + 1, xs], r[ys, xs + bpp], r[ys, xs]
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        k = ft[ys]
        pred = np.where(k == 0, 0, np.where(k == 1, a, np.where(k == 2, b, np.where(k == 3, (a + b) >> 1, paeth))))
        r[ys + 1, xs + bpp] = (x[ys, xs] + pred) & 255
    return r[1:, bpp:].astype(np.uint8)


def pixels(f, rows):
    """uint8 [H, W, 3] or [H, W]: the palette lookup, alpha dropped; raises Refused(CORRUPT) on a palette index past the PLTE entries"""
    h, w, ct, d = f["height"], f["width"], f["color_type"], f["depth"]
    if ct == 3:
        bits = np.unpackbits(rows, axis=1).reshape(h, -1, d)[:, :w]
        idx = (bits * (1 << np.arange(d - 1, -1, -1))).sum(axis=2)
        if idx.max() >= len(f["palette"]):
            raise _corrupt("a palette index past the PLTE entries")
        return f["palette"][idx]
    v = rows.reshape(h, w, f["channels"])
    return np.ascontiguousarray(v[:, :, :3] if ct in (2, 6) else v[:, :, 0])


def scanlines(data):
    f = parse(data)
    return f, inflate(f["idat"], f["raw_bytes"])


def decode(data):
    f, raw = scanlines(data)
    return pixels(f, unfilter(f, raw))


def status_of(data):
    try:
        decode(data)
        return 0
    except Refused as e:
        return e.status
