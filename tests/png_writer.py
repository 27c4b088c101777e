"""A PNG and deflate WRITER for the PNG decoder's fixtures and refusal files (tools/make_golden_png.py, tests/png_decode_cases.py): chunks with
their CRCs, the five row filters chosen by the caller (Pillow chooses its own), and deflate streams written token by token (stored, fixed-Huffman and
dynamic-Huffman blocks with any code lengths), which ``zlib`` cannot be made to write.  Test infrastructure; the decoder's model is
png_decode_model.py and shares nothing with this file."""
import binascii
import struct
import zlib

SIGNATURE = b"\x89PNG\r\n\x1a\n"


# ---- container ---------------------------------------------------------------------------------------------------------------------------
def chunk(ctype, body=b""):
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", binascii.crc32(ctype + body))


def ihdr(width, height, depth, color_type, interlace=0, compression=0, filter_method=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, color_type, compression, filter_method, interlace))


def split_idat(z, every=None, empty_between=False):
    """the zlib stream as IDAT chunks of ``every`` bytes (None: one chunk), with an empty IDAT behind the first when asked"""
    parts = [z] if not every else [z[k:k + every] for k in range(0, len(z), every)] or [b""]
    out = []
    for k, p in enumerate(parts):
        out.append(chunk(b"IDAT", p))
        if empty_between and k == 0:
            out.append(chunk(b"IDAT", b""))
    return out


def png(width, height, depth, color_type, z, palette=None, every=None, empty_between=False, before=(), after=(), interlace=0):
    """a whole file: IHDR, ``before`` chunks, PLTE, the IDAT run, ``after`` chunks, IEND"""
    parts = [SIGNATURE, ihdr(width, height, depth, color_type, interlace)] + list(before)
    if palette is not None:
        parts.append(chunk(b"PLTE", bytes(palette)))
    parts += split_idat(z, every, empty_between) + list(after) + [chunk(b"IEND")]
    return b"".join(parts)


def chunks_of(data):
    """[(type, body, offset of the length field)] of a well-formed file"""
    out, at = [], 8
    while at < len(data):
        n = struct.unpack(">I", data[at:at + 4])[0]
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n], at))
        at += 12 + n
    return out


def rebuild(chunks):
    """a file from [(type, body, ...)], every CRC fresh"""
    return SIGNATURE + b"".join(chunk(c[0], c[1]) for c in chunks)


def idat_of(data):
    return b"".join(c[1] for c in chunks_of(data) if c[0] == b"IDAT")


def with_idat(data, z):
    """the file with its IDAT run replaced by one chunk holding z"""
    out, done = [], False
    for c in chunks_of(data):
        if c[0] == b"IDAT":
            if not done:
                out.append((b"IDAT", z))
                done = True
        else:
            out.append(c)
    return rebuild(out)


def adler32(raw):
    return struct.pack(">I", zlib.adler32(raw))


# ---- filters -----------------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_rows(rows, bpp, filters):
    """rows: the unfiltered bytes of each row; filters[y % len(filters)] the filter type of row y -> the filtered scanlines with their filter bytes"""
    out, prev = bytearray(), bytes(len(rows[0]))
    for y, row in enumerate(rows):
        row, ft = bytes(row), filters[y % len(filters)]
        out.append(ft)
        for i, x in enumerate(row):
            a = row[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[ft]
            out.append((x - pred) & 255)
        prev = row
    return bytes(out)


def pack_indices(idx_rows, depth):
    """rows of palette indices -> rows of bytes, most significant bits first, the last byte padded with zero bits"""
    out = []
    for r in idx_rows:
        bits = "".join(format(int(v), "0%db" % depth) for v in r)
        bits += "0" * (-len(bits) % 8)
        out.append(bytes(int(bits[k:k + 8], 2) for k in range(0, len(bits), 8)))
    return out


# ---- deflate, token by token -----------------------------------------------------------------------------------------------------------------
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
ZLIB_HEADER = b"\x78\x9c"


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, count):
        """``count`` bits of value, least significant first (header fields and extra bits)"""
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """a Huffman code, most significant bit first"""
        for k in range(length - 1, -1, -1):
            self.bits(code >> k & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """{symbol: (code, length)} of the canonical code with these lengths (no validity check: refusal files need invalid sets)"""
    count = [0] * 16
    for v in lengths:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for k in range(1, 16):
        code = (code + count[k - 1]) << 1
        nxt[k] = code
    out = {}
    for s, v in enumerate(lengths):
        if v:
            out[s] = (nxt[v], v)
            nxt[v] += 1
    return out


def length_symbol(length):
    s = 28 if length == 258 else max(k for k in range(28) if _LBASE[k] <= length)
    return s, length - _LBASE[s], _LEXT[s]


def distance_symbol(dist):
    s = max(k for k in range(30) if _DBASE[k] <= dist)
    return s, dist - _DBASE[s], _DEXT[s]


def tokens_of(raw, distances, min_len=3):
    """a greedy tokeniser that looks at the given distances only: ('lit', byte) and ('match', length, distance).  A match may overlap its own output."""
    raw, out, p, n = bytes(raw), [], 0, len(raw)
    while p < n:
        best, bd = 0, 0
        for d in distances:
            if d > p:
                continue
            k = 0
            while k < 258 and p + k < n and raw[p + k] == raw[p + k - d]:
                k += 1
            if k > best:
                best, bd = k, d
        if best >= min_len:
            out.append(("match", best, bd))
            p += best
        else:
            out.append(("lit", raw[p]))
            p += 1
    return out


def write_tokens(w, tokens, lit, dist):
    """the tokens and the end-of-block symbol with the codes {symbol: (code, length)}"""
    for t in tokens:
        if t[0] == "lit":
            w.code(*lit[t[1]])
        else:
            s, extra, nbits = length_symbol(t[1])
            w.code(*lit[257 + s])
            w.bits(extra, nbits)
            s, extra, nbits = distance_symbol(t[2])
            w.code(*dist[s])
            w.bits(extra, nbits)
    w.code(*lit[256])


def fixed_block(w, tokens, final=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    write_tokens(w, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))


def stored_block(w, data, final=True, nlen=None):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
    for b in data:
        w.bits(b, 8)


def dynamic_header(w, lit_lengths, dist_lengths, cl_lengths=None, final=True, hlit=None, hdist=None, raw_cl_symbols=None):
    """BFINAL, BTYPE 2, HLIT, HDIST, HCLEN, the code-length code and the code lengths, each sent as itself (no repeat codes) unless
    ``raw_cl_symbols`` gives the (symbol, extra bits value) sequence to send instead.  ``cl_lengths``: the 19 lengths of the code-length code
    (default: a complete code over the lengths that occur)."""
    seq = list(lit_lengths) + list(dist_lengths)
    symbols = raw_cl_symbols if raw_cl_symbols is not None else [(v, None) for v in seq]
    if cl_lengths is None:
        used = sorted({s for s, _ in symbols})
        cl_lengths = [0] * 19
        # a complete code over `used`: lengths ceil(log2) with the Kraft sum filled up by shortening the first ones
        n = len(used)
        if n == 1:
            used.append((used[0] + 1) % 19)
            n = 2
        k = (n - 1).bit_length()
        short = (1 << k) - n                                    # that many symbols get k - 1 bits
        for j, s in enumerate(used):
            cl_lengths[s] = k - 1 if j < short else k
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit_lengths) - 257 if hlit is None else hlit, 5)
    w.bits(len(dist_lengths) - 1 if hdist is None else hdist, 5)
    ncode = max([4] + [k + 1 for k in range(19) if cl_lengths[ORDER[k]]])
    w.bits(ncode - 4, 4)
    for k in range(ncode):
        w.bits(cl_lengths[ORDER[k]], 3)
    cl = canonical(cl_lengths)
    for s, extra in symbols:
        w.code(*cl[s])
        if s == 16:
            w.bits(extra, 2)
        elif s == 17:
            w.bits(extra, 3)
        elif s == 18:
            w.bits(extra, 7)


# a complete literal/length code over all 286 symbols: 256 literals of 9 bits (1/2), 28 symbols of 6 bits (7/16), 2 of 5 bits (1/16)
FLAT_LIT = [9] * 256 + [6] * 28 + [5] * 2
FLAT_DIST = [4] * 2 + [5] * 28                                  # and a complete distance code over all 30


def dynamic_block(w, tokens, lit_lengths=None, dist_lengths=None, final=True):
    lit_lengths = FLAT_LIT if lit_lengths is None else lit_lengths
    dist_lengths = FLAT_DIST if dist_lengths is None else dist_lengths
    dynamic_header(w, lit_lengths, dist_lengths, final=final)
    write_tokens(w, tokens, canonical(lit_lengths), canonical(dist_lengths))


def zlib_stream(body, raw, adler=None):
    return ZLIB_HEADER + body + (adler32(raw) if adler is None else adler)
