"""A numpy / plain Python restatement of what Pillow writes with ``Image.save(f, "JPEG", quality=q, optimize=..., restart_marker_rows=... /
restart_marker_blocks=...)``: tests/jpeg_model.py supplies colour conversion, DCT, quantisation, the header pieces and the Annex K tables;
this file adds what the options change.  Test infrastructure: the product never imports it.

  restart intervals  jchuff.c emit_restart: after every ``restart_interval`` MCUs but the last group the bits are padded to a byte with
                     1-bits (that byte is stuffed like any other), ``FF D0+n`` follows (n = 0..7, wrapping), and the DC prediction of every
                     component starts again at 0.  jcmarker.c writes ``DRI`` between the last DHT and SOS.
  optimize           jchuff.c's gather pass counts the symbols of the scan per table (DC differences taken with the restart rule), and
                     ``jpeg_gen_optimal_table`` builds each table; the file carries DHT DC0, AC0 (, DC1, AC1) in front of DRI / SOS.

Everything here is written block by block and symbol by symbol, as the library does it: slow and plain.
"""
from __future__ import annotations

import numpy as np

import jpeg_model as M


# ---- symbols ------------------------------------------------------------------------------------------------------------------------------
def _size(v: int) -> int:
    return int(abs(int(v))).bit_length()


def _value_bits(v: int, size: int) -> int:
    return (v - 1 if v < 0 else v) & ((1 << size) - 1)


def restart_interval(width: int, channels: int, restart_rows: int = 0, restart_blocks: int = 0) -> int:
    """MCUs per interval as jinit_c_master_control derives it: rows * MCUs per row, capped at 65535; ``restart_blocks`` as given"""
    if restart_rows:
        return min(restart_rows * (width // (16 if channels == 3 else 8)), 65535)
    return int(restart_blocks)


def symbols(coef: np.ndarray, comp: np.ndarray, restart: int = 0):
    """The scan as a list of intervals, each a list of (table id, class (0 DC / 1 AC), symbol, value bits, size) in coding order.
    coef / comp as jpeg_model.coefficients gives them (zigzag, MCU order)."""
    bpm = 6 if comp.max(initial=0) > 0 else 1
    nmcu = len(coef) // bpm
    per = restart if restart > 0 else nmcu
    out = []
    for m0 in range(0, nmcu, per):
        pred = {0: 0, 1: 0, 2: 0}
        cur = []
        for g in range(m0 * bpm, min(m0 + per, nmcu) * bpm):
            c = int(comp[g])
            t = 0 if c == 0 else 1
            blk = [int(v) for v in coef[g]]
            d = blk[0] - pred[c]
            pred[c] = blk[0]
            s = _size(d)
            cur.append((t, 0, s, _value_bits(d, s), s))
            run = 0
            for k in range(1, 64):
                v = blk[k]
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    cur.append((t, 1, 0xF0, 0, 0))
                    run -= 16
                s = _size(v)
                cur.append((t, 1, (run << 4) | s, _value_bits(v, s), s))
                run = 0
            if run:
                cur.append((t, 1, 0x00, 0, 0))
        out.append(cur)
    return out


def histograms(intervals, ntab: int):
    """freq[table id][class] = 256 counts, what jchuff.c's gather pass collects"""
    freq = [[[0] * 256, [0] * 256] for _ in range(ntab)]
    for cur in intervals:
        for t, cls, sym, _, _ in cur:
            freq[t][cls][sym] += 1
    return freq


# ---- jpeg_gen_optimal_table ---------------------------------------------------------------------------------------------------------------
def code_sizes(freq):
    """the code length of every symbol (257 entries, the pseudo-symbol last) BEFORE the 16-bit limit: jchuff.c's merge loop with its
    others[] chains and its tie rule (of equal frequencies the larger symbol number, first for c1, then for c2)"""
    f = [int(v) for v in freq] + [1]
    live = [v > 0 for v in f]
    codesize = [0] * 257
    others = [-1] * 257
    while True:
        c1 = c2 = -1
        v1 = v2 = None
        for i in range(257):
            if not live[i]:
                continue
            if v2 is None or f[i] <= v2:
                if v1 is None or f[i] <= v1:
                    c2, v2 = c1, v1
                    c1, v1 = i, f[i]
                else:
                    c2, v2 = i, f[i]
        if c2 < 0:
            break
        f[c1] += f[c2]
        live[c2] = False
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    return codesize


def gen_optimal_table(freq):
    """(bits[17], huffval bytes) of libjpeg's jpeg_gen_optimal_table for 256 symbol counts"""
    codesize = code_sizes(freq)
    top = max(max(codesize), 32)
    bits = [0] * (top + 1)
    for s in range(257):
        if codesize[s]:
            bits[codesize[s]] += 1
    i = top
    while i > 16:                                                           # Annex K.2, figure K.3
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    while i > 0 and bits[i] == 0:
        i -= 1
    if i > 0:
        bits[i] -= 1                                                        # the pseudo-symbol leaves the longest length
    order = sorted((s for s in range(256) if codesize[s]), key=lambda s: (codesize[s], s))
    return bits[:17], bytes(order)


def code_table(bits, vals):
    """symbol -> (code, length), Annex C"""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


# ---- the file -----------------------------------------------------------------------------------------------------------------------------
def segments(data: bytes):
    """[(marker, offset, total length)] of the marker segments from SOI up to and including SOS"""
    out, i = [(0xD8, 0, 2)], 2
    while True:
        marker, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        out.append((marker, i, 2 + n))
        i += 2 + n
        if marker == 0xDA:
            return out


def head(width: int, height: int, components: int, quality: int) -> bytes:
    """SOI .. SOF0"""
    full = M.header(width, height, components, quality)
    last = [s for s in segments(full) if s[0] == 0xC0][0]
    return full[:last[1] + last[2]]


def sos(components: int) -> bytes:
    full = M.header(16, 16, components, 75)
    s = segments(full)[-1]
    return full[s[1]:s[1] + s[2]]


def dht(cls: int, idx: int, bits, vals) -> bytes:
    return b"\xff\xc4" + (3 + 16 + len(vals)).to_bytes(2, "big") + bytes([cls << 4 | idx]) + bytes(bits[1:17]) + bytes(vals)


def std_tables(ntab: int):
    return [[([0] + list(M.HUFF["%s%d" % (k, t)][0]), M.HUFF["%s%d" % (k, t)][1]) for k in ("dc", "ac")] for t in range(ntab)]


def file_header(width: int, height: int, components: int, quality: int, optimize: bool = False, restart: int = 0) -> bytes:
    """what lspjpeg_header gives for a handle with these options: SOI .. SOS (with DRI), or SOI .. SOF0 with optimize"""
    out = head(width, height, components, quality)
    if optimize:
        return out
    for t, pair in enumerate(std_tables(1 if components == 1 else 2)):
        for cls, (bits, vals) in enumerate(pair):
            out += dht(cls, t, bits, vals)
    if restart:
        out += b"\xff\xdd\x00\x04" + restart.to_bytes(2, "big")
    return out + sos(components)


def scan_bytes(intervals, tables, info=None) -> bytes:
    """the entropy-coded segment without EOI; ``info`` (a dict) receives per interval its bit count and whether its padded byte was stuffed"""
    codes = [[code_table(*pair[0]), code_table(*pair[1])] for pair in tables]
    out = bytearray()
    if info is not None:
        info["bits"], info["stuffed_pad"] = [], []
    for n, cur in enumerate(intervals):
        acc = nbits = 0
        for t, cls, sym, val, size in cur:
            code, length = codes[t][cls][sym]
            acc = (acc << (length + size)) | (code << size) | val
            nbits += length + size
        pad = -nbits % 8
        acc = (acc << pad) | ((1 << pad) - 1)
        raw = acc.to_bytes((nbits + pad) // 8, "big")
        out += raw.replace(b"\xff", b"\xff\x00")
        if info is not None:
            info["bits"].append(nbits)
            info["stuffed_pad"].append(bool(pad) and raw[-1] == 0xFF)
        if n < len(intervals) - 1:
            out += bytes([0xFF, 0xD0 + (n & 7)])
    return bytes(out)


def frame_bytes(img: np.ndarray, quality: int, optimize: bool, restart: int, info=None) -> bytes:
    """everything behind file_header(...): with optimize DHT .. SOS, then the scan and EOI"""
    comps = 1 if img.ndim == 2 else 3
    ntab = 1 if comps == 1 else 2
    coef, comp = M.coefficients(img, quality)
    iv = symbols(coef, comp, restart)
    out = b""
    if optimize:
        freq = histograms(iv, ntab)
        tables = [[gen_optimal_table(freq[t][0]), gen_optimal_table(freq[t][1])] for t in range(ntab)]
        for t in range(ntab):
            for cls in (0, 1):
                out += dht(cls, t, *tables[t][cls])
        if restart:
            out += b"\xff\xdd\x00\x04" + restart.to_bytes(2, "big")
        out += sos(comps)
        if info is not None:
            info["freq"], info["tables"] = freq, tables
    else:
        tables = std_tables(ntab)
    return out + scan_bytes(iv, tables, info) + b"\xff\xd9"


def encode(img: np.ndarray, quality: int = 75, optimize: bool = False, restart_interval: int = 0, info=None) -> bytes:
    """the bytes Image.fromarray(img).save(f, "JPEG", quality=, optimize=, restart_marker_blocks=restart_interval) writes"""
    img = np.asarray(img)
    comps = 1 if img.ndim == 2 else 3
    return file_header(img.shape[1], img.shape[0], comps, quality, optimize, restart_interval) + frame_bytes(img, quality, optimize, restart_interval, info)


def parse_dht(data: bytes):
    """{(class, id): (bits[17], huffval)} of a file's DHT segments"""
    out = {}
    for marker, at, n in segments(data):
        if marker != 0xC4:
            continue
        i, end = at + 4, at + n
        while i < end:
            tc = data[i]
            bits = [0] + list(data[i + 1:i + 17])
            k = sum(bits)
            out[(tc >> 4, tc & 15)] = (bits, bytes(data[i + 17:i + 17 + k]))
            i += 17 + k
    return out


# ---- the picture that sends a table through the 16-bit limit -----------------------------------------------------------------------------
def limiter_image(quality: int = 25, nsym: int = 17, width_blocks: int = 64) -> np.ndarray:
    """A grey picture whose every block holds one AC coefficient, an exact multiple of its quantiser, so that it codes one chosen (run, size)
    symbol and EOB; the symbols occur 1, 2, 3, 5, 8 ... times.  With the pseudo-symbol's 1 every merge then joins the tree so far to the next
    symbol, so unlimited Huffman codes grow one bit per symbol: 17 symbols under EOB reach 18 bits."""
    lq, _ = M.quant_tables(quality)
    picks = [(k, mag) for mag in (1, 2) for k in range(1, 16)][:nsym]       # zigzag position (run = k - 1) and magnitude (size 1 or 2)
    fib = [1, 2]
    while len(fib) < nsym:
        fib.append(fib[-1] + fib[-2])
    blocks = []
    yy, xx = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    for (k, mag), count in zip(picks, fib):
        nat = int(M.ZIGZAG[k])
        u, v = nat // 8, nat % 8
        cu, cv = (np.sqrt(0.5) if u == 0 else 1.0), (np.sqrt(0.5) if v == 0 else 1.0)
        amp = mag * int(lq[nat])
        px = 128 + 0.25 * cu * cv * amp * np.cos((2 * yy + 1) * u * np.pi / 16) * np.cos((2 * xx + 1) * v * np.pi / 16)
        blocks += [np.clip(np.rint(px), 0, 255).astype(np.uint8)] * count
    rows = -(-len(blocks) // width_blocks)
    blocks += [np.full((8, 8), 128, np.uint8)] * (rows * width_blocks - len(blocks))
    return np.block([[blocks[r * width_blocks + c] for c in range(width_blocks)] for r in range(rows)])


def make_image(r: dict) -> np.ndarray:
    """jpeg_model.make_image plus the recipe kind "limiter" """
    if r["kind"] == "limiter":
        img = limiter_image(r["quality"], r["nsym"], r["w"] // 8)
        assert img.shape == (r["h"], r["w"])
        return img
    return M.make_image(r)
