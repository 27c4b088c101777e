"""A strict RIFF / AVI 1.0 walker for the tests of livespeechportraits_amd/video.py.  It shares no code with the writer: it reads the
bytes the way the format documents them and raises AviError on anything that does not add up.  parse() returns a dict:

    avih, streams [ {strh, strf} ], chunks [ (fourcc, offset relative to the 'movi' fourcc, payload bytes) ], index [ (ckid, flags, offset,
    length) ], first_chunk (file offset of the first chunk), video [payloads], audio (the stream's samples: float32 or int16), audio_counts
    (samples per audio chunk)
"""
import numpy as np


class AviError(ValueError):
    pass


def _need(cond, what):
    if not cond:
        raise AviError(what)


def _u32(b, at):
    _need(at + 4 <= len(b), "file ends inside a 32-bit field at %d" % at)
    return int.from_bytes(b[at:at + 4], "little")


def _u16(b, at):
    return int.from_bytes(b[at:at + 2], "little")


def _s32(b, at):
    return int.from_bytes(b[at:at + 4], "little", signed=True)


def _children(b, start, end):
    """(fourcc, payload start, payload size) of the chunks that tile [start, end) exactly, pad bytes checked"""
    out, at = [], start
    while at < end:
        _need(at % 2 == 0, "chunk starts at odd offset %d" % at)
        _need(at + 8 <= end, "chunk header at %d crosses the end of its list (%d)" % (at, end))
        cc, n = bytes(b[at:at + 4]), _u32(b, at + 4)
        _need(at + 8 + n <= end, "chunk %r at %d (%d bytes) crosses the end of its list (%d)" % (cc, at, n, end))
        out.append((cc, at + 8, n))
        at += 8 + n
        if n % 2:
            _need(at < end, "chunk %r at %d lacks its pad byte" % (cc, at - 8 - n))
            _need(b[at] == 0, "pad byte at %d is 0x%02x" % (at, b[at]))
            at += 1
    _need(at == end, "children end at %d, their list at %d" % (at, end))
    return out


def _list_of(b, child, kind):
    cc, at, n = child
    _need(cc == b"LIST", "expected a LIST, found %r" % cc)
    _need(n >= 4 and bytes(b[at:at + 4]) == kind, "expected LIST %r, found %r" % (kind, bytes(b[at:at + 4])))
    return at + 4, at + n


def _avih(b, at):
    names = ("dwMicroSecPerFrame", "dwMaxBytesPerSec", "dwPaddingGranularity", "dwFlags", "dwTotalFrames", "dwInitialFrames", "dwStreams",
             "dwSuggestedBufferSize", "dwWidth", "dwHeight")
    d = {n: _u32(b, at + 4 * k) for k, n in enumerate(names)}
    d["dwReserved"] = [_u32(b, at + 40 + 4 * k) for k in range(4)]
    return d


def _strh(b, at):
    d = {"fccType": bytes(b[at:at + 4]), "fccHandler": bytes(b[at + 4:at + 8]), "dwFlags": _u32(b, at + 8), "wPriority": _u16(b, at + 12),
         "wLanguage": _u16(b, at + 14)}
    for k, n in enumerate(("dwInitialFrames", "dwScale", "dwRate", "dwStart", "dwLength", "dwSuggestedBufferSize", "dwQuality", "dwSampleSize")):
        d[n] = _u32(b, at + 16 + 4 * k)
    d["rcFrame"] = tuple(int.from_bytes(b[at + 48 + 2 * k:at + 50 + 2 * k], "little", signed=True) for k in range(4))
    return d


def _bitmapinfo(b, at):
    return {"biSize": _u32(b, at), "biWidth": _s32(b, at + 4), "biHeight": _s32(b, at + 8), "biPlanes": _u16(b, at + 12), "biBitCount": _u16(b, at + 14),
            "biCompression": bytes(b[at + 16:at + 20]), "biSizeImage": _u32(b, at + 20), "biXPelsPerMeter": _s32(b, at + 24),
            "biYPelsPerMeter": _s32(b, at + 28), "biClrUsed": _u32(b, at + 32), "biClrImportant": _u32(b, at + 36)}


def _waveformat(b, at):
    return {"wFormatTag": _u16(b, at), "nChannels": _u16(b, at + 2), "nSamplesPerSec": _u32(b, at + 4), "nAvgBytesPerSec": _u32(b, at + 8),
            "nBlockAlign": _u16(b, at + 12), "wBitsPerSample": _u16(b, at + 14), "cbSize": _u16(b, at + 16)}


def parse(data):
    b = bytes(data)
    _need(len(b) >= 12 and b[:4] == b"RIFF" and b[8:12] == b"AVI ", "not a RIFF 'AVI ' file")
    _need(_u32(b, 4) == len(b) - 8, "RIFF size %d, file has %d bytes after it (trailing or missing bytes)" % (_u32(b, 4), len(b) - 8))
    _need(_u32(b, 4) <= 2 ** 31 - 1, "RIFF size past 2^31 - 1")
    top = _children(b, 12, len(b))
    _need([c[0] for c in top] == [b"LIST", b"LIST", b"idx1"], "top level is %r, expected hdrl, movi, idx1" % [c[0] for c in top])

    # ---- hdrl
    h0, h1 = _list_of(b, top[0], b"hdrl")
    hdrl = _children(b, h0, h1)
    _need(len(hdrl) >= 2 and hdrl[0][0] == b"avih", "hdrl does not start with avih")
    _need(hdrl[0][2] == 56, "avih has %d bytes, not 56" % hdrl[0][2])
    avih = _avih(b, hdrl[0][1])
    streams = []
    for child in hdrl[1:]:
        s0, s1 = _list_of(b, child, b"strl")
        parts = _children(b, s0, s1)
        _need([p[0] for p in parts] == [b"strh", b"strf"], "strl holds %r" % [p[0] for p in parts])
        _need(parts[0][2] == 56, "strh has %d bytes, not 56" % parts[0][2])
        strh = _strh(b, parts[0][1])
        if strh["fccType"] == b"vids":
            _need(parts[1][2] == 40, "video strf has %d bytes, not 40" % parts[1][2])
            strf = _bitmapinfo(b, parts[1][1])
        elif strh["fccType"] == b"auds":
            _need(parts[1][2] == 18, "audio strf has %d bytes, not 18" % parts[1][2])
            strf = _waveformat(b, parts[1][1])
        else:
            raise AviError("stream type %r" % strh["fccType"])
        streams.append({"strh": strh, "strf": strf})
    _need(avih["dwStreams"] == len(streams), "avih says %d streams, hdrl holds %d" % (avih["dwStreams"], len(streams)))
    _need(len(streams) in (1, 2) and streams[0]["strh"]["fccType"] == b"vids", "stream 0 must be the video")
    _need(len(streams) == 1 or streams[1]["strh"]["fccType"] == b"auds", "stream 1 must be the audio")

    # ---- movi
    m0, m1 = _list_of(b, top[1], b"movi")
    fourcc_at = m0 - 4
    movi = _children(b, m0, m1)
    chunks = [(cc, at - 8 - fourcc_at, b[at:at + n]) for cc, at, n in movi]
    for cc, _, _ in chunks:
        _need(cc in ((b"00dc", b"01wb") if len(streams) == 2 else (b"00dc",)), "chunk %r in movi" % cc)
    video = [p for cc, _, p in chunks if cc == b"00dc"]
    sound = [p for cc, _, p in chunks if cc == b"01wb"]

    # ---- idx1
    _, i0, n = top[2]
    _need(n % 16 == 0, "idx1 has %d bytes" % n)
    index = [(bytes(b[i0 + 16 * k:i0 + 16 * k + 4]), _u32(b, i0 + 16 * k + 4), _u32(b, i0 + 16 * k + 8), _u32(b, i0 + 16 * k + 12)) for k in range(n // 16)]
    _need(len(index) == len(chunks), "%d index entries for %d chunks" % (len(index), len(chunks)))
    for k, ((ckid, flags, off, length), (cc, rel, payload)) in enumerate(zip(index, chunks)):
        _need(flags == 0x10, "index entry %d has flags 0x%x" % (k, flags))
        at = fourcc_at + off
        _need(at + 8 <= m1 and bytes(b[at:at + 4]) == ckid, "index entry %d points at %r, not %r" % (k, bytes(b[at:at + 4]), ckid))
        _need(_u32(b, at + 4) == length, "index entry %d says %d bytes, the chunk %d" % (k, length, _u32(b, at + 4)))
        _need(ckid == cc and off == rel, "index entry %d is not chunk %d of movi" % (k, k))
    if chunks:
        _need(index[0][2] == 4, "the first chunk is at offset %d of movi, not 4" % index[0][2])

    # ---- counts the headers promise
    vh = streams[0]["strh"]
    _need(avih["dwTotalFrames"] == len(video), "dwTotalFrames %d, movi holds %d frames" % (avih["dwTotalFrames"], len(video)))
    _need(vh["dwLength"] == len(video), "video dwLength %d, movi holds %d frames" % (vh["dwLength"], len(video)))
    largest_v = max([len(p) for p in video], default=0)
    largest_a = max([len(p) for p in sound], default=0)
    _need(vh["dwSuggestedBufferSize"] >= largest_v, "video dwSuggestedBufferSize %d below the largest chunk %d" % (vh["dwSuggestedBufferSize"], largest_v))
    _need(avih["dwSuggestedBufferSize"] >= max(largest_v, largest_a), "avih dwSuggestedBufferSize below the largest chunk")
    audio, counts = None, []
    if len(streams) == 2:
        ah, wf = streams[1]["strh"], streams[1]["strf"]
        align = wf["nBlockAlign"]
        _need(align > 0 and all(len(p) % align == 0 for p in sound), "an audio chunk is no whole number of blocks")
        counts = [len(p) // align for p in sound]
        _need(ah["dwLength"] == sum(counts), "audio dwLength %d, movi holds %d samples" % (ah["dwLength"], sum(counts)))
        _need(ah["dwSuggestedBufferSize"] >= largest_a, "audio dwSuggestedBufferSize %d below the largest chunk %d" % (ah["dwSuggestedBufferSize"], largest_a))
        _need(len(sound) == len(video), "%d audio chunks for %d frames" % (len(sound), len(video)))
        _need([cc for cc, _, _ in chunks] == [b"01wb", b"00dc"] * len(video), "audio and video are not interleaved per frame")
        _need((wf["wFormatTag"], wf["wBitsPerSample"]) in ((3, 32), (1, 16)), "audio format %d with %d bits" % (wf["wFormatTag"], wf["wBitsPerSample"]))
        audio = np.frombuffer(b"".join(sound), dtype="<f4" if wf["wFormatTag"] == 3 else "<i2")
    return {"avih": avih, "streams": streams, "chunks": chunks, "index": index, "first_chunk": m0, "video": video, "audio": audio,
            "audio_counts": counts}
