"""A numpy / plain Python restatement of what Pillow writes with ``Image.save(f, "JPEG", quality=q, subsampling=s, ...)`` for a picture of
ANY size: tests/jpeg_model.py supplies colour conversion, DCT, quantisation and the header pieces, tests/jpeg_options_model.py the Huffman
tables, the restart intervals and the scan; this file adds libjpeg's edge handling and the three chroma layouts.  Test infrastructure: the
product never imports it.

With luma factors (hs, vs) = (2, 2) for 4:2:0, (2, 1) for 4:2:2, (1, 1) for 4:4:4:
  MCU grid      colour: ceil(W / 8hs) x ceil(H / 8vs) MCUs of hs * vs luma blocks (row-major), Cb, Cr.  Grey: a non-interleaved scan, one block
                per MCU, ceil(W / 8) x ceil(H / 8) of them.
  columns       jcsample.c expand_right_edge: the last pixel of a row repeated, BEFORE downsampling; the bias patterns run on into the padding.
                h2v2: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2 ...; h2v1: (a + b + bias) >> 1, bias 0, 1, 0, 1 ...; 4:4:4: the sample itself.
  rows          jcprepct.c: the last pixel row repeated up to a multiple of vs only; then the plane is downsampled; then the last row of each
                COMPONENT plane is repeated down to the block grid.
  dummy blocks  jccoefct.c: a luma block of an edge MCU whose column >= ceil(W / 8) or row >= ceil(H / 8) is not transformed: its AC
                coefficients are 0 and its DC is the quantised DC of the block before it in the MCU (which may itself be such a block).
"""
from __future__ import annotations

import numpy as np

import jpeg_model as M
import jpeg_options_model as O

FACTORS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
FORMATS = ("4:4:4", "4:2:2", "4:2:0", "grey")
COMP, BX, BY, DUMMY, PREV, DCSRC = range(6)                     # the columns of block_map


def factors(fmt: str):
    """(components, hs, vs) of one of FORMATS"""
    return (1, 1, 1) if fmt == "grey" else (3,) + FACTORS[fmt]


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def grid(w: int, h: int, comps: int, hs: int, vs: int):
    """(MCUs per row, MCU rows, blocks per MCU)"""
    if comps == 1:
        return cdiv(w, 8), cdiv(h, 8), 1
    return cdiv(w, 8 * hs), cdiv(h, 8 * vs), hs * vs + 2


def restart_interval(w: int, comps: int, hs: int, restart_rows: int = 0, restart_blocks: int = 0) -> int:
    if restart_rows:
        return min(restart_rows * grid(w, 8, comps, hs, 1)[0], 65535)
    return int(restart_blocks)


def block_map(w: int, h: int, comps: int, hs: int, vs: int) -> np.ndarray:
    """int32 [blocks, 6] in coding order: component, block column and row in the component's plane, dummy (0 / 1), the index of the previous
    block of the component (-1 for the first), the index of the block whose quantised DC this one carries (itself unless dummy).  Written
    MCU by MCU, as jccoefct.c walks them."""
    mx, my, bpm = grid(w, h, comps, hs, vs)
    lbx, lby = cdiv(w, 8), cdiv(h, 8)
    rows, last = [], {}
    for m in range(mx * my):
        x, y = m % mx, m // mx
        src = -1
        for j in range(bpm):
            g = m * bpm + j
            if comps == 1 or j < hs * vs:
                c, bx, by = 0, x * hs + j % hs, y * vs + j // hs
                dummy = int(bx >= lbx or by >= lby)
            else:
                c, bx, by, dummy = j - hs * vs + 1, x, y, 0
            if not dummy:
                src = g
            assert src >= m * bpm
            rows.append((c, bx, by, dummy, last.get(c, -1), src))
            last[c] = g
    return np.array(rows, np.int32)


def _pad_cols(p: np.ndarray, width: int) -> np.ndarray:
    return np.concatenate([p, np.repeat(p[:, -1:], width - p.shape[1], 1)], 1)


def _pad_rows(p: np.ndarray, height: int) -> np.ndarray:
    return np.concatenate([p, np.repeat(p[-1:], height - p.shape[0], 0)], 0)


def planes(img: np.ndarray, hs: int, vs: int):
    """the component planes the DCT sees (int64, not yet level-shifted), padded to whole MCUs"""
    h, w = img.shape[:2]
    if img.ndim == 2:
        return [_pad_rows(_pad_cols(img.astype(np.int64), cdiv(w, 8) * 8), cdiv(h, 8) * 8)]
    mx, my, _ = grid(w, h, 3, hs, vs)
    y, cb, cr = (_pad_rows(_pad_cols(p, mx * 8 * hs), cdiv(h, vs) * vs) for p in M.rgb_to_ycc(img))
    out = [y]
    for c in (cb, cr):
        if (hs, vs) == (2, 2):
            s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
            c = (s + np.tile(np.array([1, 2], np.int64), s.shape[1] // 2)[None, :]) >> 2
        elif (hs, vs) == (2, 1):
            s = c[:, 0::2] + c[:, 1::2]
            c = (s + np.tile(np.array([0, 1], np.int64), s.shape[1] // 2)[None, :]) >> 1
        out.append(c)
    return [_pad_rows(out[0], my * 8 * vs)] + [_pad_rows(c, my * 8) for c in out[1:]]


def coefficients(img: np.ndarray, quality: int, hs: int = 2, vs: int = 2):
    """(zigzag coefficients [blocks, 64] in coding order, component per block); dummy blocks as jccoefct.c fills them"""
    h, w = img.shape[:2]
    comps = 1 if img.ndim == 2 else 3
    if comps == 1:
        hs = vs = 1
    bm = block_map(w, h, comps, hs, vs)
    lq, cq = M.quant_tables(quality)
    q = []
    for c, p in enumerate(planes(img, hs, vs)):
        b = M._blocks(p - 128)
        z = M.quantise(M.fdct_islow(b), lq if c == 0 else cq)
        q.append(z.reshape(z.shape[:2] + (64,))[..., M.ZIGZAG])
    coef = np.zeros((len(bm), 64), np.int64)
    for g, (c, bx, by, dummy, _, src) in enumerate(bm):
        if dummy:
            coef[g, 0] = coef[src, 0]
        else:
            coef[g] = q[c][by, bx]
    return coef, bm[:, COMP].astype(np.int64)


def symbols(coef: np.ndarray, comp: np.ndarray, bpm: int, restart: int = 0):
    """jpeg_options_model.symbols for any number of blocks per MCU"""
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
            s = O._size(d)
            cur.append((t, 0, s, O._value_bits(d, s), s))
            run = 0
            for k in range(1, 64):
                v = blk[k]
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    cur.append((t, 1, 0xF0, 0, 0))
                    run -= 16
                s = O._size(v)
                cur.append((t, 1, (run << 4) | s, O._value_bits(v, s), s))
                run = 0
            if run:
                cur.append((t, 1, 0x00, 0, 0))
        out.append(cur)
    return out


def file_header(w: int, h: int, comps: int, quality: int, hs: int, vs: int, optimize: bool = False, restart: int = 0) -> bytes:
    """what lspjpeg_header gives for a format handle: SOI .. SOS (with DRI), or SOI .. SOF0 with optimize; SOF0 carries the true W and H and
    the luma sampling byte hs << 4 | vs"""
    out = bytearray(O.file_header(w, h, comps, quality, optimize, restart))
    at = [s for s in O.segments(bytes(out) + (O.sos(comps) if optimize else b"")) if s[0] == 0xC0][0][1]
    out[at + 11] = (hs << 4 | vs) if comps == 3 else 0x11
    return bytes(out)


def encode(img: np.ndarray, quality: int = 75, fmt: str = "4:2:0", optimize: bool = False, restart_rows: int = 0, restart_blocks: int = 0, info=None) -> bytes:
    """the bytes Image.fromarray(img).save(f, "JPEG", quality=, subsampling=, optimize=, restart_marker_rows= / restart_marker_blocks=) writes"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    comps, hs, vs = factors("grey" if img.ndim == 2 else fmt)
    restart = restart_interval(w, comps, hs, restart_rows, restart_blocks)
    ntab = 1 if comps == 1 else 2
    coef, comp = coefficients(img, quality, hs, vs)
    iv = symbols(coef, comp, grid(w, h, comps, hs, vs)[2], restart)
    out = file_header(w, h, comps, quality, hs, vs, optimize, restart)
    if optimize:
        freq = O.histograms(iv, ntab)
        tables = [[O.gen_optimal_table(freq[t][0]), O.gen_optimal_table(freq[t][1])] for t in range(ntab)]
        for t in range(ntab):
            for cls in (0, 1):
                out += O.dht(cls, t, *tables[t][cls])
        if restart:
            out += b"\xff\xdd\x00\x04" + restart.to_bytes(2, "big")
        out += O.sos(comps)
    else:
        tables = O.std_tables(ntab)
    if info is not None:
        info["restart"], info["blocks"], info["intervals"] = restart, len(coef), len(iv)
    return out + O.scan_bytes(iv, tables) + b"\xff\xd9"


# ---- the fixture recipes -----------------------------------------------------------------------------------------------------------------------
def make_image(r: dict) -> np.ndarray:
    return M.make_image(r)


def fixture_case(row) -> dict:
    """a row of tests/golden/jpeg_geometry.json (h, w, format, quality, optimize, restart_rows, restart_blocks, kind) -> name, options, recipe"""
    h, w, fmt, q, o, rows, blocks, kind = row
    return {"name": "%s_%s_%dx%d_q%d_o%d_r%d_b%d" % (kind, fmt.replace(":", ""), h, w, q, o, rows, blocks), "format": fmt, "quality": q, "optimize": o,
            "restart_rows": rows, "restart_blocks": blocks, "recipe": dict(kind=kind, h=h, w=w, channels=1 if fmt == "grey" else 3, seed=1000 + 7 * h + 3 * w, value=90)}


def load_fixtures(golden_dir: str):
    """(meta, [case dicts], {name: Pillow's file})"""
    import json
    import os
    meta = json.load(open(os.path.join(golden_dir, "jpeg_geometry.json")))
    z = np.load(os.path.join(golden_dir, "jpeg_geometry.npz"))
    data, ends = z["data"].tobytes(), [0] + [int(v) for v in z["ends"]]
    cases = [fixture_case(row) for row in meta["cases"]]
    return meta, cases, {c["name"]: data[ends[k]:ends[k + 1]] for k, c in enumerate(cases)}


def pillow_bytes(Image, img: np.ndarray, quality: int, fmt: str, optimize=False, restart_rows=0, restart_blocks=0) -> bytes:
    import io
    b = io.BytesIO()
    kw = {} if img.ndim == 2 else dict(subsampling=PILLOW_SUBSAMPLING[fmt])
    Image.fromarray(img).save(b, "JPEG", quality=quality, optimize=bool(optimize), restart_marker_rows=restart_rows, restart_marker_blocks=restart_blocks, **kw)
    return b.getvalue()
