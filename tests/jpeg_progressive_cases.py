"""The fixtures of the progressive JPEG tests (tests/golden/jpeg_prog.{json,npz}, jpeg_prog_512.npz: tools/make_golden_jpeg_progressive.py) and
the files the tests edit out of them: one per refusal include/lspjpegdec.h lists under LSPJPEG_DEC_FLAG_PROGRESSIVE.  Test infrastructure, shared
by the CPU and the GPU file."""
import functools
import json
import os

import numpy as np

import jpeg_decode_model as D
import jpeg_progressive_model as P
from conftest import GOLDEN


@functools.lru_cache(maxsize=None)
def fixtures():
    """(meta, {name: progressive file}, {name: baseline twin}, {name: pixels})"""
    with open(os.path.join(GOLDEN, "jpeg_prog.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(GOLDEN, "jpeg_prog.npz"))
    files = {k[:-4]: z[k].tobytes() for k in z.files if k.endswith(".jpg")}
    twins = {k[:-5]: z[k].tobytes() for k in z.files if k.endswith(".twin")}
    pixels = {k[:-3]: z[k] for k in z.files if k.endswith(".px")}
    return meta, files, twins, pixels


@functools.lru_cache(maxsize=None)
def frames_512():
    """({name: progressive file}, {name: baseline twin}) of the constant frame and the four candidates; the candidates' twins are
    candidate_{j}_512_q95 of tests/golden/jpeg_dec_512.npz"""
    z = np.load(os.path.join(GOLDEN, "jpeg_prog_512.npz"))
    files = {k[:-4]: z[k].tobytes() for k in z.files if k.endswith(".jpg")}
    twins = {k[:-5]: z[k].tobytes() for k in z.files if k.endswith(".twin")}
    base = np.load(os.path.join(GOLDEN, "jpeg_dec_512.npz"))
    for c in fixtures()[0]["frames"]:
        if "twin" in c:
            twins[c["name"]] = base[c["twin"] + ".jpg"].tobytes()
    return files, twins


def small_names():
    return [c["name"] for c in fixtures()[0]["cases"]]


def find(part):
    return next(n for n in small_names() if part in n)


# ---- editing ---------------------------------------------------------------------------------------------------------------------------
def patched(data, at, new):
    b = bytearray(data)
    b[at:at + len(new)] = new
    return bytes(b)


def refusals():
    """[(what, file, status under the flag)]: each made by editing fixture bytes.  Pillow's colour files hold ten scans: 0 DC of all components
    0/1, 1 Y 1-5 0/2, 2 Cr 1-63 0/1, 3 Cb 1-63 0/1, 4 Y 6-63 0/2, 5 Y 1-63 2/1, 6 DC 1/0, 7 Cr 1-63 1/0, 8 Cb 1-63 1/0, 9 Y 1-63 1/0; the
    three bytes before a scan's data are Ss, Se and Ah << 4 | Al."""
    _, files, _, _ = fixtures()
    c420 = files[find("_420_plain_40x72_")]
    rst = files[find("_420_rstr_40x72_")]
    sc = P.parse(c420)["scans"]
    assert [(s["ss"], s["se"], s["ah"], s["al"]) for s in sc] == [(0, 0, 0, 1), (1, 5, 0, 2), (1, 63, 0, 1), (1, 63, 0, 1), (6, 63, 0, 2), (1, 63, 2, 1), (0, 0, 1, 0),
                                                                  (1, 63, 1, 0), (1, 63, 1, 0), (1, 63, 1, 0)]
    U, C = D.UNSUPPORTED, D.CORRUPT
    out = [("a bogus progression (Y 1-5 first coded at Al 1, refined from Al 2)", patched(c420, sc[1]["begin"] - 1, b"\x01"), U),
           ("a scan removed (incomplete)", c420[:sc[8]["end"]] + b"\xff\xd9", U)]
    dq = c420.index(b"\xff\xdb")
    dqt = c420[dq:dq + 2 + int.from_bytes(c420[dq + 2:dq + 4], "big")]
    out.append(("a DQT after the first SOS", c420[:sc[0]["end"]] + dqt + c420[sc[0]["end"]:], U))
    sos = sc[1]["begin"] - 10                                              # ff da 00 08 01 <id> <tables> Ss Se AhAl
    assert c420[sos:sos + 5] == b"\xff\xda\x00\x08\x01"
    ids = [c[0] for c in P.parse(c420)["comps"]]
    two = b"\xff\xda\x00\x0a\x02" + bytes([ids[0], 0x00, ids[1], 0x00]) + c420[sos + 7:sos + 10]
    out.append(("an AC scan with two components", c420[:sos] + two + c420[sc[1]["begin"]:], C))
    out.append(("Se < Ss", patched(c420, sc[1]["begin"] - 3, b"\x06\x05"), C))
    out.append(("Al = 14", patched(c420, sc[0]["begin"] - 1, b"\x0e"), C))
    third = P.parse(rst)["scans"][2]
    at = rst.index(b"\xff\xd0", third["begin"], third["end"])
    out.append(("a wrong RSTn inside the third scan", patched(rst, at + 1, b"\xd1"), C))
    out.append(("a scan cut short", c420[:sc[4]["end"] - 6] + c420[sc[4]["end"]:], C))
    relabelled = c420                                                      # every luma AC scan on table id 3: DHT class 1 id 0 -> id 3, the SOS alike
    for s in sc:
        if s["ss"] and s["comps"] == [0]:
            dht = relabelled.rindex(b"\xff\xc4", 0, s["begin"])
            assert relabelled[dht + 4] == 0x10 and relabelled[s["begin"] - 4] == 0x00
            relabelled = patched(patched(relabelled, dht + 4, b"\x13"), s["begin"] - 4, b"\x03")
    out.append(("(control) table id 3 decodes", relabelled, 0))
    out.append(("SOF0 with the progressive scans", patched(c420, c420.index(b"\xff\xc2") + 1, b"\xc0"), U))
    return out
