"""The fixtures of the JPEG decoder's tests (tests/golden/jpeg_dec.{json,npz}, jpeg_dec_512.npz: tools/make_golden_jpeg_decode.py) and the
files the tests edit out of them: one per refusal of include/lspjpegdec.h.  Test infrastructure, shared by the CPU and the GPU file."""
import functools
import json
import os

import numpy as np

import jpeg_decode_model as D
import jpeg_model as M
from conftest import GOLDEN


@functools.lru_cache(maxsize=None)
def fixtures():
    """(meta, {name: bytes}, {name: pixels})"""
    with open(os.path.join(GOLDEN, "jpeg_dec.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(GOLDEN, "jpeg_dec.npz"))
    files = {k[:-4]: z[k].tobytes() for k in z.files if k.endswith(".jpg")}
    pixels = {k[:-3]: z[k] for k in z.files if k.endswith(".px")}
    return meta, files, pixels


@functools.lru_cache(maxsize=None)
def frames_512():
    """{name: bytes} of the twelve 512^2 files"""
    z = np.load(os.path.join(GOLDEN, "jpeg_dec_512.npz"))
    return {k[:-4]: z[k].tobytes() for k in z.files}


def small_names():
    return [c["name"] for c in fixtures()[0]["cases"]]


def find(part):
    return next(n for n in small_names() if part in n)


# ---- editing ---------------------------------------------------------------------------------------------------------------------------
def segments(data):
    """[(marker, offset of the 0xFF, total bytes)] of the header's marker segments, SOS included"""
    out, i = [], 2
    while True:
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        out.append((m, i, 2 + n))
        i += 2 + n
        if m == 0xDA:
            return out


def segment(data, marker, nth=0):
    return [s for s in segments(data) if s[0] == marker][nth]


def patched(data, at, new):
    b = bytearray(data)
    b[at:at + len(new)] = new
    return bytes(b)


def pack_bits(symbols):
    """[(value, length)] -> a scan: MSB first, padded with 1-bits, 0xFF stuffed"""
    acc = n = 0
    for v, l in symbols:
        acc, n = (acc << l) | v, n + l
    pad = (-n) % 8
    acc, n = (acc << pad) | ((1 << pad) - 1), n + pad
    return acc.to_bytes(n // 8, "big").replace(b"\xff", b"\xff\x00")


def refusals():
    """[(what, file, status)]: every refusal the header lists, each made by editing fixture bytes (progressive and CMYK come from Pillow)"""
    meta, files, _ = fixtures()
    c420 = files[find("_420_40x72_")]
    rst = files[find("_rstr_40x72_")]
    grey_nodht = files[find("_grey_40x72_") + "_nodht"]
    U, C = D.UNSUPPORTED, D.CORRUPT
    out = [("progressive", files["refused_progressive"], U), ("4 components (CMYK)", files["refused_cmyk"], U)]
    sof = segment(c420, 0xC0)[1]
    sos = segment(c420, 0xDA)
    for m, what in ((0xC1, "extended sequential (SOF1)"), (0xC9, "arithmetic coding (SOF9)"), (0xC3, "lossless (SOF3)")):
        out.append((what, patched(c420, sof + 1, bytes([m])), U))
    out.append(("12-bit precision", patched(c420, sof + 4, b"\x0c"), U))
    _, dq, dqn = segment(c420, 0xDB)
    wide = b"\xff\xdb" + (3 + 128).to_bytes(2, "big") + bytes([0x10 | (c420[dq + 4] & 15)]) + b"".join(b"\x00" + bytes([v]) for v in c420[dq + 5:dq + 69])
    out.append(("16-bit DQT", c420[:dq] + wide + c420[dq + dqn:], U))
    out.append(("luma sampled 1x2", patched(c420, sof + 11, b"\x12"), U))
    out.append(("luma sampled 4x1", patched(c420, sof + 11, b"\x41"), U))
    out.append(("chroma sampled 2x1", patched(c420, sof + 14, b"\x21"), U))
    one_scan = b"\xff\xda\x00\x08\x01" + c420[sos[1] + 5:sos[1] + 7] + b"\x00\x3f\x00"
    out.append(("several scans (SOS of one component)", c420[:sos[1]] + one_scan + c420[sos[1] + sos[2]:], U))
    out.append(("spectral selection 0..5", patched(c420, sos[1] + sos[2] - 2, b"\x05"), U))
    rgb = patched(patched(patched(c420, sof + 10, b"R"), sof + 13, b"G"), sof + 16, b"B")
    rgb = patched(patched(patched(rgb, sos[1] + 5, b"R"), sos[1] + 7, b"G"), sos[1] + 9, b"B")
    out.append(("component ids R G B", rgb, U))
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    out.append(("Adobe APP14 transform 0", c420[:2] + adobe + c420[2:], U))
    out.append(("fill byte before EOI", c420[:-2] + b"\xff" + c420[-2:], U))
    out.append(("COM marker inside the scan", c420[:-2] + b"\xff\xfe\x00\x02" + c420[-2:], U))
    out.append(("RST0 without DRI", c420[:-2] + b"\xff\xd0" + c420[-2:], U))
    # CORRUPT
    first_rst = rst.index(b"\xff\xd0", segment(rst, 0xDA)[1])
    out.append(("a wrong RSTn", patched(rst, first_rst + 1, b"\xd1"), C))
    out.append(("a missing RSTn", rst[:first_rst] + rst[first_rst + 2:], C))
    out.append(("an RSTn too many", rst[:-2] + b"\xff" + bytes([0xD0 + (len(D.parse(rst)["segments"]) - 1) % 8]) + rst[-2:], C))
    out.append(("the file ends inside the scan", c420[:len(c420) - 30], C))
    out.append(("the scan ends early (EOI kept)", c420[:-12] + c420[-2:], C))
    out.append(("whole bytes left over", c420[:-2] + b"\x00\x00\x00" + c420[-2:], C))
    _, dh, dhn = segment(c420, 0xC4, 0)                                    # DC table 0: every symbol becomes 12
    out.append(("a DC size above 11", patched(c420, dh + 21, b"\x0c" * (dhn - 21)), C))
    _, ah, ahn = segment(c420, 0xC4, 1)                                    # AC table 0: every symbol becomes run 0, size 11
    out.append(("an AC size above 10", patched(c420, ah + 21, b"\x0b" * (ahn - 21)), C))
    # one grey 8x8 block on Annex K's tables, its scan written here
    gsof = segment(grey_nodht, 0xC0)[1]
    head = patched(grey_nodht, gsof + 5, b"\x00\x08\x00\x08")[:D.parse(grey_nodht)["scan_begin"]]
    dco, dsi = M._CODES["dc0"]
    aco, asi = M._CODES["ac0"]
    zrl = (int(aco[0xF0]), int(asi[0xF0]))
    ok = head + pack_bits([(int(dco[0]), int(dsi[0])), zrl, zrl, zrl, (int(aco[0xE1]), int(asi[0xE1])), (1, 1)]) + b"\xff\xd9"
    out.append(("(control) a coefficient at index 63 decodes", ok, 0))
    past = head + pack_bits([(int(dco[0]), int(dsi[0])), zrl, zrl, zrl, (int(aco[0xF1]), int(asi[0xF1])), (1, 1)]) + b"\xff\xd9"
    out.append(("a coefficient index past 63", past, C))
    out.append(("a code that is in no table", head + b"\xff\x00" * 3 + b"\xff\xd9", C))      # sixteen 1-bits: longer than any DC code
    out.append(("no quantisation table", patched(c420, dq + 1, b"\xfe"), C))                   # the DQT becomes a comment
    return out
