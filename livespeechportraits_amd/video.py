"""The video of demo.py:275-285 (``write_video_with_audio``) as a Motion-JPEG AVI: the JPEG files the render loop already encodes on the
device (jpeg.py, byte-identical to Pillow's ``pred_<n>.jpg``) are the video chunks, and the clip's 16 kHz waveform is the audio stream.

The reference reads every ``pred_<n>.jpg`` back, re-encodes it (DIVX) and muxes ``librosa.output.write_wav``'s float WAV in with an external
program's ``-codec copy``; its audio stream is therefore float PCM, which is why ``f32`` is the default here.  We write ``MJPG`` holding the
files themselves: no second lossy generation.

Layout (AVI 1.0, little-endian, no OpenDML)::

    RIFF 'AVI ' / LIST 'hdrl' (avih, LIST 'strl' video [, LIST 'strl' audio]) / LIST 'movi' (['01wb'] '00dc' per frame) / 'idx1'

``AviWriter`` is host code (no device needed): the headers, the index, the 2 GiB rule, and ``append_jpegs`` which builds a batch's part
of 'movi' from complete JPEG files.  ``DeviceMuxer`` builds the same bytes on the device (include/lspavi.h) behind ``lspjpeg_encode`` and
brings them over in one copy; ``AviWriter.append_fragment`` takes them.  No player or demuxer can be run where this is built, so the
container is pinned on the strict parser of tests/avi_parser.py and on Pillow decoding every chunk: it is *player-unpinned*.

``AviReader`` is the way back: a host-side parser of exactly these files, whose ``frames()`` decodes the chunks on the device
(jpeg.JpegDecoder) to the pixels Pillow returns for them.
"""
from __future__ import annotations

import ctypes
import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np

AUDIO_FORMATS = {"f32": (3, 4), "s16": (1, 2)}                  # name -> (wFormatTag, bytes per sample)
# which route the render loops take when ``video`` is given: "device" (DeviceMuxer + append_fragment) or "host" (JpegEncoder.collect +
# append_jpegs).  Set from profiles/avi_time.txt, see DESIGN.md section 20.
DEFAULT_VIDEO_ROUTE = "device"
# which route LivePortraitPool records by when ``record_route`` is not given: "device" (DeviceMultiMuxer, one lspavi_pack_multi per group of
# frames) or "host" (JpegEncoder + append_jpegs per session).  By section 20's rule, see DESIGN.md section 21.
DEFAULT_LIVE_RECORD_ROUTE = "device"


class AviFull(RuntimeError):
    """the append would take the file past ``max_bytes``: nothing was written; close this file and start another"""


def frame_sample(frame: int, rate: int, fps: int) -> int:
    """the first audio sample of ``frame``: frame k carries samples [k * rate // fps, (k + 1) * rate // fps)"""
    return int(frame) * int(rate) // int(fps)


def pcm16(x: np.ndarray) -> np.ndarray:
    """the ``s16`` rule: rintf(x * 32767.0f) clamped to +-32767, NaN as 0"""
    v = np.rint(np.asarray(x, np.float32) * np.float32(32767.0))
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, -32767, 32767))
    return v.astype("<i2")


def jpeg_geometry(data: bytes) -> Tuple[int, int, int]:
    """(width, height, components) of a baseline JPEG file, from its SOF0 segment"""
    at = 2
    while at + 4 <= len(data) and data[at] == 0xFF:
        marker, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        if marker == 0xC0:
            return int.from_bytes(data[at + 7:at + 9], "big"), int.from_bytes(data[at + 5:at + 7], "big"), data[at + 9]
        if marker == 0xDA:
            break
        at += 2 + n
    raise ValueError("no SOF0 segment before the scan: not a baseline JPEG file")


class AviWriter:
    """One Motion-JPEG AVI file.  ``channels`` 3 (colour files) or 1 (grayscale); ``audio_rate`` None for a file without an audio stream.
    The header is written with placeholders at construction; ``close()`` writes 'idx1' and every size and count.  A context manager."""

    def __init__(self, path: str, width: int, height: int, channels: int = 3, fps: int = 60, audio_rate: Optional[int] = 16000,
                 audio_format: str = "f32", max_bytes: int = 2 ** 31 - 1):
        if channels not in (1, 3):
            raise ValueError("channels must be 3 (colour) or 1 (grayscale)")
        if audio_format not in AUDIO_FORMATS:
            raise ValueError("audio_format must be one of %s" % sorted(AUDIO_FORMATS))
        if not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535 and int(fps) >= 1 and (audio_rate is None or int(audio_rate) >= 1)):
            raise ValueError("width, height, fps and audio_rate must be positive (width and height below 65536)")
        if not 0 < int(max_bytes) <= 2 ** 31 - 1:
            raise ValueError("max_bytes must be in 1..2**31 - 1 (AVI 1.0: no OpenDML)")
        self.path, self.width, self.height, self.channels, self.fps = path, int(width), int(height), int(channels), int(fps)
        self.audio_rate = None if audio_rate is None else int(audio_rate)
        self.audio_format = audio_format if self.audio_rate is not None else None
        self.max_bytes = int(max_bytes)
        self.nframes = self.nsamples = 0
        self._movi = 0                                          # bytes of chunks in 'movi' so far
        self._index = bytearray()
        self._largest_video = self._largest_audio = 0
        self._header_len = 326 if self.has_audio else 224       # bytes up to the first chunk
        assert len(self._header()) == self._header_len
        if self._riff_size(0, 0) > self.max_bytes:
            raise AviFull("max_bytes=%d does not hold an empty file" % self.max_bytes)
        self._f = open(path, "wb")
        self._f.write(self._header())

    # ---- layout ------------------------------------------------------------------------------------------------------------
    @property
    def has_audio(self) -> bool:
        return self.audio_rate is not None

    @property
    def bytes_per_sample(self) -> int:
        return AUDIO_FORMATS[self.audio_format][1] if self.has_audio else 0

    def span(self, frame0: int, nframes: int) -> Tuple[int, int]:
        """audio samples [first, last) of frames frame0 .. frame0 + nframes - 1 (0, 0 without audio)"""
        if not self.has_audio:
            return 0, 0
        return frame_sample(frame0, self.audio_rate, self.fps), frame_sample(frame0 + nframes, self.audio_rate, self.fps)

    def _riff_size(self, more_bytes: int, more_chunks: int) -> int:
        """the RIFF chunk's size field if ``more_bytes`` of chunks in ``more_chunks`` chunks were appended and the file closed"""
        return self._header_len - 8 + self._movi + more_bytes + 8 + len(self._index) + 16 * more_chunks

    def room_for(self, nbytes: int, nchunks: int) -> bool:
        """would ``nbytes`` more bytes of 'movi' in ``nchunks`` chunks still close within ``max_bytes``?  (what append_fragment checks
        before it writes; a caller that cannot know a fragment's size yet asks with its worst case)"""
        return self._riff_size(int(nbytes), int(nchunks)) <= self.max_bytes

    def _header(self) -> bytes:
        """everything up to the first chunk of 'movi', from the current counts"""
        W, H, fps, n = self.width, self.height, self.fps, self.nframes
        bits = 24 if self.channels == 3 else 8
        strl = [struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, 1, fps, 0, n, self._largest_video, 0xFFFFFFFF, 0, 0, 0, W, H),
                struct.pack("<IiiHH4sIiiII", 40, W, H, 1, bits, b"MJPG", W * H * bits // 8, 0, 0, 0, 0)]
        lists = [_list(b"strl", _chunk(b"strh", strl[0]) + _chunk(b"strf", strl[1]))]
        if self.has_audio:
            tag, align = AUDIO_FORMATS[self.audio_format]
            strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, self.audio_rate, 0, self.nsamples, self._largest_audio,
                               0xFFFFFFFF, align, 0, 0, 0, 0)
            strf = struct.pack("<HHIIHHH", tag, 1, self.audio_rate, self.audio_rate * align, align, 8 * align, 0)
            lists.append(_list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf)))
        rate = -(-self._movi * fps // n) if n else 0
        avih = struct.pack("<14I", int(round(1e6 / fps)), rate, 0, 0x110, n, 0, len(lists), max(self._largest_video, self._largest_audio), W, H, 0, 0, 0, 0)
        hdrl = _list(b"hdrl", _chunk(b"avih", avih) + b"".join(lists))
        body = b"AVI " + hdrl + b"LIST" + struct.pack("<I", 4 + self._movi) + b"movi"
        return b"RIFF" + struct.pack("<I", self._riff_size(0, 0)) + body

    # ---- appending ---------------------------------------------------------------------------------------------------------
    def append_fragment(self, data, index, nframes: int, nsamples: int, largest_video: int, largest_audio: int = 0) -> None:
        """Append bytes built elsewhere (DeviceMuxer.collect(), or another writer's append_jpegs): ``data`` the chunks of ``nframes`` frames
        in file order, ``index`` uint32 [chunks][4] (ckid, flags, offset relative to ``data``'s start, unpadded length)."""
        if self._f is None:
            raise ValueError("the file is closed")
        data = memoryview(data).cast("B") if not isinstance(data, np.ndarray) else memoryview(np.ascontiguousarray(data, np.uint8)).cast("B")
        index = np.ascontiguousarray(index, dtype="<u4").reshape(-1, 4)
        nframes, nsamples = int(nframes), int(nsamples)
        first, last = self.span(self.nframes, nframes)
        if index.shape[0] != nframes * (2 if self.has_audio else 1):
            raise ValueError("%d index entries for %d frames of a file %s audio" % (index.shape[0], nframes, "with" if self.has_audio else "without"))
        if nsamples != last - first:
            raise ValueError("frames %d..%d carry %d samples, the fragment has %d" % (self.nframes, self.nframes + nframes - 1, last - first, nsamples))
        if len(data) & 1:
            raise ValueError("a fragment's length is even (chunks are padded)")
        if nframes and (int(index[0, 2]) != 0 or int(index[-1, 2]) + 8 + int(index[-1, 3]) + (int(index[-1, 3]) & 1) != len(data)):
            raise ValueError("the index does not span the fragment")
        if self._riff_size(len(data), index.shape[0]) > self.max_bytes:
            raise AviFull("%d more bytes take the file past max_bytes=%d: close it and start another" % (len(data), self.max_bytes))
        index = index.copy()
        index[:, 2] += np.uint32(4 + self._movi)                # 'idx1' offsets count from the 'movi' fourcc
        self._f.write(data)
        self._index += index.tobytes()
        self._movi += len(data)
        self.nframes += nframes
        self.nsamples += nsamples
        self._largest_video = max(self._largest_video, int(largest_video))
        self._largest_audio = max(self._largest_audio, int(largest_audio))

    def build_fragment(self, files: Sequence[bytes], samples=None):
        """What append_fragment takes, for the next ``len(files)`` frames, built on the host from complete JPEG files."""
        files = [bytes(f) for f in files]
        first, last = self.span(self.nframes, len(files))
        if self.has_audio:
            if samples is None:
                raise ValueError("this file has an audio stream: frames %d..%d need %d samples" % (self.nframes, self.nframes + len(files) - 1, last - first))
            samples = np.ascontiguousarray(np.asarray(samples), dtype=np.float32).reshape(-1)
            if samples.shape[0] != last - first:
                raise ValueError("frames %d..%d carry %d samples, got %d" % (self.nframes, self.nframes + len(files) - 1, last - first, samples.shape[0]))
            pcm = samples.astype("<f4") if self.audio_format == "f32" else pcm16(samples)
        elif samples is not None:
            raise ValueError("this file has no audio stream")
        out, index = bytearray(), []
        largest_video = largest_audio = 0
        for k, f in enumerate(files):
            if len(f) < 4 or f[:2] != b"\xff\xd8" or f[-2:] != b"\xff\xd9":
                raise ValueError("frame %d is not a complete JPEG file (SOI .. EOI)" % (self.nframes + k))
            if jpeg_geometry(f) != (self.width, self.height, self.channels):
                raise ValueError("frame %d is %dx%d with %d components, the file %dx%d with %d" % ((self.nframes + k,) + jpeg_geometry(f) +
                                                                                                  (self.width, self.height, self.channels)))
            if self.has_audio:
                a, b = self.span(self.nframes + k, 1)
                piece = pcm[a - first:b - first].tobytes()
                index.append((0x62773130, 0x10, len(out), len(piece)))
                out += b"01wb" + struct.pack("<I", len(piece)) + piece
                largest_audio = max(largest_audio, len(piece))
            index.append((0x63643030, 0x10, len(out), len(f)))
            out += b"00dc" + struct.pack("<I", len(f)) + f + (b"\0" if len(f) & 1 else b"")
            largest_video = max(largest_video, len(f))
        return bytes(out), np.array(index, dtype="<u4").reshape(-1, 4), len(files), last - first, largest_video, largest_audio

    def append_jpegs(self, files: Sequence[bytes], samples=None):
        """Append complete JPEG files (Pillow's, JpegEncoder.encode's, LivePortraitPool.tick(jpeg_quality=...)'s) as the next frames;
        ``samples``: float32, exactly the samples those frames carry (``span``).  Returns the fragment it appended."""
        fragment = self.build_fragment(files, samples)
        self.append_fragment(*fragment)
        return fragment

    # ---- closing -----------------------------------------------------------------------------------------------------------
    def close(self) -> None:
        if self._f is None:
            return
        f, self._f = self._f, None
        try:
            f.write(b"idx1" + struct.pack("<I", len(self._index)) + bytes(self._index))
            f.seek(0)
            f.write(self._header())
        finally:
            f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def _list(kind: bytes, body: bytes) -> bytes:
    return b"LIST" + struct.pack("<I", 4 + len(body)) + kind + body


def write_avi(path: str, jpegs: Sequence[bytes], waveform=None, fps: int = 60, audio_rate: int = 16000, audio_format: str = "f32",
              batch: int = 64) -> int:
    """Write files the caller already holds (``render_frames(..., jpeg_quality=75)``, or with a ``jpeg.JpegOptions``: every chunk is a whole file,
    optimised tables and restart markers included) as one AVI; ``waveform``: the clip's float32 samples at
    ``audio_rate`` (None: no audio stream), at least ``len(jpegs) * audio_rate // fps`` of them.  Returns the frame count."""
    jpegs = list(jpegs)
    if not jpegs:
        raise ValueError("no frames: the geometry of the file comes from the first one")
    w, h, c = jpeg_geometry(bytes(jpegs[0]))
    wave = None if waveform is None else np.asarray(waveform, dtype=np.float32).reshape(-1)
    with AviWriter(path, w, h, c, fps, audio_rate if wave is not None else None, audio_format) as out:
        for k in range(0, len(jpegs), batch):
            part = jpegs[k:k + batch]
            a, b = out.span(k, len(part))
            if wave is not None and b > wave.shape[0]:
                raise ValueError("%d frames need %d samples, the waveform has %d" % (k + len(part), b, wave.shape[0]))
            out.append_jpegs(part, None if wave is None else wave[a:b])
        return out.nframes


class AviError(ValueError):
    """the file is not an AVI ``AviReader`` reads"""


class AviReader:
    """The way back from the files ``AviWriter`` and the live recorder write: a host-side RIFF parser for AVI 1.0 with 'idx1' (one 'MJPG'
    video stream, optionally one PCM or float audio stream, no OpenDML) and, through ``frames``, the device decode of its chunks
    (jpeg.JpegDecoder: the pixels Pillow returns for each chunk).  Anything else is refused with an ``AviError``.  The file is read once,
    at construction; chunks are handed out by their index entries.  Chunks without DHT segments are fine: the decoder falls back on
    the standard tables."""

    def __init__(self, path: str):
        self.path = path
        with open(path, "rb") as f:
            b = self._data = f.read()
        need = self._need
        need(len(b) >= 12 and b[:4] == b"RIFF" and b[8:12] == b"AVI ", "not a RIFF 'AVI ' file")
        need(self._u32(4) + 8 == len(b), "the RIFF size does not match the file (truncated, or an OpenDML file continued in further RIFF chunks)")
        top = self._children(12, len(b))
        need([c[0] for c in top] == [b"LIST", b"LIST", b"idx1"], "top level is %r, expected LIST hdrl, LIST movi, idx1" % [c[0] for c in top])
        h0, h1 = self._list(top[0], b"hdrl")
        hdrl = self._children(h0, h1)
        need(len(hdrl) >= 2 and hdrl[0][0] == b"avih" and hdrl[0][2] >= 40, "hdrl does not start with avih")
        streams = [c for c in hdrl[1:] if c[0] == b"LIST" and bytes(b[c[1]:c[1] + 4]) == b"strl"]
        need(len(streams) in (1, 2) and self._u32(hdrl[0][1] + 24) == len(streams), "one video stream and at most one audio stream are read (the file has %d)" % len(streams))
        # video
        strh, strf = self._strl(streams[0])
        need(bytes(b[strh:strh + 4]) == b"vids", "stream 0 is not the video")
        need(bytes(b[strf + 16:strf + 20]) == b"MJPG", "video compression %r: only MJPG is read" % bytes(b[strf + 16:strf + 20]))
        scale, rate = self._u32(strh + 20), self._u32(strh + 24)
        need(scale >= 1 and rate >= 1 and rate % scale == 0, "a frame rate of %d / %d is no whole number" % (rate, scale))
        self.fps = rate // scale
        self.width, self.height = self._u32(strf + 4), self._u32(strf + 8)
        self.channels = 3 if int.from_bytes(b[strf + 14:strf + 16], "little") == 24 else 1
        # audio
        self.audio_rate = self.audio_format = None
        if len(streams) == 2:
            strh, strf = self._strl(streams[1])
            need(bytes(b[strh:strh + 4]) == b"auds", "stream 1 is not audio")
            tag, nch, bits = (int.from_bytes(b[strf + o:strf + o + 2], "little") for o in (0, 2, 14))
            fmt = {(3, 32): "f32", (1, 16): "s16"}.get((tag, bits))
            need(fmt is not None and nch == 1, "audio format tag %d with %d bits and %d channels: mono float32 or int16 PCM is read" % (tag, bits, nch))
            self.audio_rate, self.audio_format = self._u32(strf + 4), fmt
        # movi + idx1
        m0, m1 = self._list(top[1], b"movi")
        _, i0, n = top[2]
        need(n % 16 == 0, "idx1 has %d bytes" % n)
        self._video, self._audio = [], []
        for k in range(n // 16):
            ckid, off, length = bytes(b[i0 + 16 * k:i0 + 16 * k + 4]), self._u32(i0 + 16 * k + 8), self._u32(i0 + 16 * k + 12)
            at = m0 - 4 + off                                  # offsets count from the 'movi' fourcc
            need(at + 8 + length <= m1 and bytes(b[at:at + 4]) == ckid and self._u32(at + 4) == length, "index entry %d does not point at its chunk" % k)
            if ckid == b"00dc":
                self._video.append((at + 8, length))
            elif ckid == b"01wb" and self.audio_rate is not None:
                self._audio.append((at + 8, length))
            else:
                raise AviError("index entry %d names chunk %r" % (k, ckid))
        self.nframes = len(self._video)

    # ---- RIFF ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _need(cond, what):
        if not cond:
            raise AviError(what)

    def _u32(self, at: int) -> int:
        self._need(at + 4 <= len(self._data), "the file ends inside a 32-bit field at %d" % at)
        return int.from_bytes(self._data[at:at + 4], "little")

    def _children(self, start: int, end: int):
        out, at = [], start
        while at < end:
            self._need(at + 8 <= end, "a chunk header at %d crosses the end of its list" % at)
            cc, n = bytes(self._data[at:at + 4]), self._u32(at + 4)
            self._need(at + 8 + n <= end, "chunk %r at %d crosses the end of its list" % (cc, at))
            out.append((cc, at + 8, n))
            at += 8 + n + (n & 1)
        return out

    def _list(self, child, kind: bytes):
        cc, at, n = child
        self._need(cc == b"LIST" and n >= 4 and bytes(self._data[at:at + 4]) == kind, "expected LIST %r" % kind)
        return at + 4, at + n

    def _strl(self, child):
        parts = {cc: (at, n) for cc, at, n in self._children(child[1] + 4, child[1] + child[2])}
        self._need(b"strh" in parts and b"strf" in parts and parts[b"strh"][1] >= 48 and parts[b"strf"][1] >= 16, "a stream list without strh / strf")
        return parts[b"strh"][0], parts[b"strf"][0]

    # ---- content ------------------------------------------------------------------------------------------------------------
    def jpeg(self, i: int) -> bytes:
        """video chunk i: one complete JPEG file"""
        at, n = self._video[i]
        return bytes(self._data[at:at + n])

    def audio(self) -> Optional[np.ndarray]:
        """the audio stream's samples as written (float32 or int16), None without one"""
        if self.audio_rate is None:
            return None
        raw = b"".join(bytes(self._data[at:at + n]) for at, n in self._audio)
        return np.frombuffer(raw, dtype="<f4" if self.audio_format == "f32" else "<i2")

    def frames(self, start: int = 0, stop: Optional[int] = None, decoder=None, batch: int = 64, parallel: bool = False):
        """Yields frames start .. stop - 1 as uint8 device tensors ([H, W, 3], or [H, W] for a grayscale file), decoded ``batch`` chunks per
        call of ``decoder`` (a jpeg.JpegDecoder; by default one on cuda:0 sized for this file).  A chunk the decoder refuses raises
        jpeg.JpegError.  ``parallel``: the decoder this call makes decodes inside each frame in parallel (jpeg.JpegDecoder's ``parallel``; a
        ``decoder`` passed in decides for itself)."""
        start, stop, _ = slice(start, stop).indices(self.nframes)
        if decoder is None:
            from .jpeg import JpegDecoder
            decoder = JpegDecoder("cuda:0", max_side=max(self.width, self.height, 1), max_batch=batch, parallel=parallel)
        for k in range(start, stop, batch):
            for frame in decoder.decode([self.jpeg(i) for i in range(k, min(k + batch, stop))]):
                yield frame


class _MuxBuffers:
    """What the two device muxers share: the library, the encoder, the JPEG header on the device (padded to whole dwords), the fragment
    buffer ``_out``, the workspace ``_ws``, status + index in one tensor ``_meta`` with its pinned mirror, and the pinned mirror of the bytes."""

    def __init__(self, encoder, rate: int, fps: int):
        from . import _native as N
        if encoder.max_batch > N.AVI_MAX_BATCH:
            raise ValueError("the muxer packs at most %d frames per call (encoder.max_batch = %d)" % (N.AVI_MAX_BATCH, encoder.max_batch))
        self.N, self.lib, self.enc = N, N.load(), encoder
        self.rate, self.fps, self.device = int(rate), int(fps), encoder.device

    def _allocate(self, capacity: int, ws_bytes: int, meta_rows: int) -> None:
        """``meta_rows``: rows of 4 words, the status block(s) first, then 2 * max_batch index rows"""
        import torch
        self.capacity, self._ws_bytes = int(capacity), int(ws_bytes)
        if self.capacity == 0 or self._ws_bytes == 0:
            raise ValueError("lspavi: geometry, batch, rate or fps out of range")
        dev, header = self.device, self.enc.header
        self._header = torch.frombuffer(bytearray(header + b"\0" * (-len(header) % 4)), dtype=torch.uint8).to(dev)
        self._out = torch.empty(self.capacity, dtype=torch.uint8, device=dev)
        self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=dev)
        self._meta = torch.empty((meta_rows, 4), dtype=torch.int32, device=dev)
        self._meta_host = torch.empty((meta_rows, 4), dtype=torch.int32, pin_memory=True)
        self._host = torch.empty(0, dtype=torch.uint8)

    def _is_wave(self, t) -> bool:
        """a contiguous 1-D float32 tensor on this device?"""
        import torch
        return isinstance(t, torch.Tensor) and t.dim() == 1 and t.dtype == torch.float32 and t.device == self.device and t.is_contiguous()

    def _fetch(self, total: int, stream) -> np.ndarray:
        """exactly the first ``total`` bytes of ``_out`` in one copy on ``stream``, waited for: a view of pinned memory"""
        import torch
        if self._host.numel() < total:
            self._host = torch.empty(max(total, 2 * self._host.numel()), dtype=torch.uint8, pin_memory=True)
        with torch.cuda.stream(stream):
            self._host[:total].copy_(self._out[:total], non_blocking=True)
        stream.synchronize()
        return self._host.numpy()[:total]


class DeviceMuxer(_MuxBuffers):
    """``lspjpeg_encode`` then ``lspavi_pack`` (include/lspavi.h) on the current stream: a batch of uint8 device frames becomes its part of
    the file's 'movi' list on the device -- chunk headers, the JPEG header, the entropy-coded bytes, pad bytes and the interleaved audio -- and
    crosses PCIe in ONE copy with its index entries.  Owns the fragment buffer, workspace, index and status tensors and their pinned mirrors;
    uses ``encoder``'s output slab, so the encoder must not be used on its own while a batch is in flight here."""

    def __init__(self, encoder, audio_format: Optional[str] = "f32", rate: int = 16000, fps: int = 60):
        if audio_format is not None and audio_format not in AUDIO_FORMATS:
            raise ValueError("audio_format must be one of %s or None" % sorted(AUDIO_FORMATS))
        super().__init__(encoder, rate, fps)
        self.audio_format = audio_format
        B, lib = encoder.max_batch, self.lib
        fmt = self.N.AVI_AUDIO_FORMATS[audio_format]
        self._allocate(lib.lspavi_capacity_bytes(len(encoder.header), encoder.capacity, B, fmt, self.rate, self.fps), lib.lspavi_workspace_bytes(B),
                       1 + 2 * B)                               # row 0: the status block; then the index
        self._pending = None

    def submit(self, frames, frame0: int, audio_dev=None) -> None:
        """Enqueue the encode, the pack and the copy of the status block and the index on the current stream.  ``frame0``: the clip's
        number of frames[0]; ``audio_dev``: the CLIP's float32 waveform on the device (None: no audio chunks).  A waveform too short for the
        batch's last sample is refused by lspavi_pack on the host (LspaviError): no pack is enqueued and nothing is left to collect."""
        import torch
        if self._pending is not None:
            raise RuntimeError("collect() the previous batch first: the muxer's buffers are still in use")
        c = ctypes.c_void_p
        fmt, wave, nwave = 0, None, 0
        if audio_dev is not None:
            if self.audio_format is None:
                raise ValueError("this muxer was made without an audio format")
            if not self._is_wave(audio_dev):
                raise ValueError("audio_dev must be a contiguous 1-D float32 tensor on %s" % self.device)
            fmt, wave, nwave = self.N.AVI_AUDIO_FORMATS[self.audio_format], audio_dev.data_ptr(), audio_dev.shape[0]
        b = self.enc.enqueue(frames)
        stream = torch.cuda.current_stream(self.device)
        dst, sizes = self.enc.slab
        with torch.cuda.device(self.device):
            self.N.check_avi(self.lib.lspavi_pack(
                c(self._header.data_ptr()), len(self.enc.header), c(dst.data_ptr()), self.enc.capacity, c(sizes.data_ptr()), b,
                c(wave), nwave, int(frame0), self.rate, self.fps, fmt, c(self._out.data_ptr()), self.capacity,
                c(self._meta[1:].data_ptr()), c(self._meta.data_ptr()), c(self._ws.data_ptr()), self._ws_bytes, c(stream.cuda_stream)))
            n = 1 + (2 * b if fmt else b)
            self._meta_host[:n].copy_(self._meta[:n], non_blocking=True)
        self._pending = (b, fmt != 0, int(frame0), stream)

    def collect(self):
        """Wait for the submitted batch, copy exactly the fragment's bytes in one copy; returns ``(data, index, nframes, nsamples,
        largest_video, largest_audio)``, what AviWriter.append_fragment takes.  ``data`` is a view of pinned memory, valid until the next
        collect()."""
        if self._pending is None:
            raise RuntimeError("nothing submitted")
        b, audio, frame0, stream = self._pending
        self._pending = None
        stream.synchronize()
        meta = self._meta_host.numpy().view(np.uint32)
        total, nchunk, largest_video, largest_audio = (int(v) for v in meta[0])
        if nchunk != (2 * b if audio else b) or not 0 < total <= self.capacity or total & 1:
            raise RuntimeError("lspavi_pack returned %d bytes in %d chunks for %d frames (capacity %d)" % (total, nchunk, b, self.capacity))
        data = self._fetch(total, stream)
        nsamples = frame_sample(frame0 + b, self.rate, self.fps) - frame_sample(frame0, self.rate, self.fps) if audio else 0
        return data, meta[1:1 + nchunk].copy(), b, nsamples, largest_video, largest_audio


def clip_audio(video: AviWriter, audio, device):
    """The render loops' ``audio`` argument (the CLIP's float32 waveform at the writer's rate: a tensor anywhere, or an array) as
    (contiguous device tensor, host array); (None, None) for a writer without an audio stream.  Frame k of the FILE carries samples
    [k * rate // fps, (k + 1) * rate // fps) of it."""
    import torch
    if not video.has_audio:
        if audio is not None:
            raise ValueError("audio given, but the AviWriter was made with audio_rate=None")
        return None, None
    if audio is None:
        raise ValueError("the AviWriter has an audio stream: pass the clip's waveform as audio (or make the writer with audio_rate=None)")
    t = audio if isinstance(audio, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(audio), dtype=np.float32))
    t = t.detach().reshape(-1).to(torch.float32)
    return t.to(device).contiguous(), t.cpu().numpy()


class VideoSink:
    """What one lane of a render loop puts behind its generator when ``video`` is given: submit() a batch of uint8 device frames on the
    current stream, collect() it into the writer.  ``route`` "device": DeviceMuxer + append_fragment (one copy per batch); "host":
    JpegEncoder.submit / collect + append_jpegs (one copy per frame, the fragment built on the host).  Both write the same bytes.
    ``quality``: 1..100 or a ``jpeg.JpegOptions`` (optimised tables, restart intervals)."""

    def __init__(self, video: AviWriter, size, quality, device, max_batch: int, audio_dev=None, audio_host=None, route: Optional[str] = None):
        from .jpeg import JpegEncoder
        route = route or DEFAULT_VIDEO_ROUTE
        if route not in ("device", "host"):
            raise ValueError("video_route must be 'device' or 'host'")
        size = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        if (size[1], size[0]) != (video.width, video.height):
            raise ValueError("the frames are %dx%d, the AviWriter %dx%d" % (size[1], size[0], video.width, video.height))
        self.video, self.route, self.audio_dev, self.audio_host = video, route, audio_dev, audio_host
        self.enc = JpegEncoder(size, video.channels, quality, device, max_batch=max_batch)
        self.mux = DeviceMuxer(self.enc, video.audio_format, video.audio_rate or 16000, video.fps) if route == "device" else None
        self._frame0 = None

    def submit(self, frames, frame0: int) -> None:
        if self.mux is not None:
            self.mux.submit(frames, frame0, self.audio_dev)
        else:
            a, b = self.video.span(frame0, int(frames.shape[0]))
            if self.audio_host is not None and b > self.audio_host.shape[0]:
                raise ValueError("frames %d..%d need %d samples, the waveform has %d" % (frame0, frame0 + frames.shape[0] - 1, b, self.audio_host.shape[0]))
            self.enc.submit(frames)
        self._frame0 = int(frame0)

    def collect(self) -> int:
        """the submitted batch, appended to the writer (in the order of the calls: the caller drains its lanes oldest first)"""
        if self._frame0 != self.video.nframes:
            raise RuntimeError("batch of frame %s collected when the file holds %d frames: fragments must be appended in frame order" % (self._frame0, self.video.nframes))
        if self.mux is not None:
            fragment = self.mux.collect()
            self.video.append_fragment(*fragment)
            return fragment[2]
        files = self.enc.collect()
        a, b = self.video.span(self._frame0, len(files))
        self.video.append_jpegs(files, None if self.audio_host is None else self.audio_host[a:b])
        return len(files)


# ---- live sessions: one file per session, fragments of many files from one batch ------------------------------
def live_ring_samples(lag_frames: int, max_tick_samples: int, rate: int = 16000, fps: int = 60) -> int:
    """Samples a live session's audio ring must hold so that the span of every frame a tick emits is still in it.  ``lag_frames``: how
    far the oldest frame a tick can emit lies behind the audio pushed BEFORE that tick (the audio models' lookahead plus the landmark
    filters' radius); 4 frames on top for the mel windows' rounding and the one-sample slack of ``sample0``; then the tick's own push."""
    return int(max_tick_samples) + (int(lag_frames) + 4) * -(-int(rate) // int(fps))


class RingBook:
    """The host's account of one audio ring: stream sample i lives at ``i % ring_samples``; ``pushed`` samples have been appended."""

    def __init__(self, ring_samples: int):
        if int(ring_samples) < 1:
            raise ValueError("ring_samples must be >= 1")
        self.ring_samples, self.pushed = int(ring_samples), 0

    @property
    def avail(self) -> Tuple[int, int]:
        """the stream samples [begin, end) the ring holds"""
        return max(0, self.pushed - self.ring_samples), self.pushed

    def push(self, n: int) -> np.ndarray:
        """account for ``n`` more samples: the ring positions they go to, in order"""
        n = int(n)
        if not 0 <= n <= self.ring_samples:
            raise ValueError("a push of %d samples does not fit a ring of %d" % (n, self.ring_samples))
        at = (self.pushed + np.arange(n, dtype=np.int64)) % self.ring_samples
        self.pushed += n
        return at

    def positions(self, first: int, last: int) -> np.ndarray:
        """the ring positions of stream samples [first, last); refused when the ring does not hold them all"""
        begin, end = self.avail
        if not begin <= first <= last <= end:
            raise ValueError("samples %d..%d are not in the ring, which holds %d..%d" % (first, last, begin, end))
        return np.arange(first, last, dtype=np.int64) % self.ring_samples


class LiveRecording:
    """One file of one live session.  The file's frame 0 is the stream's frame ``base``; its frame k carries the stream samples
    ``sample0 + [s(k), s(k + 1))`` with ``sample0 = s(base)`` and s = frame_sample -- AviWriter.span's rule on the file's own numbering,
    at most one sample off the stream's own s(base + k).  ``make_room`` is the rollover rule, the same for every route."""

    def __init__(self, sid: int, which: str, writer: AviWriter, on_full, stream_frame: int):
        self.sid, self.which, self.on_full = sid, which, on_full
        self._start(writer, stream_frame)

    def _start(self, writer: AviWriter, stream_frame: int) -> None:
        if writer.nframes or writer.nsamples:
            raise ValueError("session %d: the %s writer already holds %d frames; a recording starts an empty file" % (self.sid, self.which, writer.nframes))
        self.writer, self.base = writer, int(stream_frame)
        self.sample0 = frame_sample(self.base, writer.audio_rate, writer.fps) if writer.has_audio else 0

    def span(self, count: int) -> Tuple[int, int]:
        """stream samples [first, last) of the file's next ``count`` frames ((0, 0) without audio)"""
        a, b = self.writer.span(self.writer.nframes, count)
        return (self.sample0 + a, self.sample0 + b) if self.writer.has_audio else (0, 0)

    def worst_case(self, count: int, frame_bytes: int) -> Tuple[int, int]:
        """(bytes, chunks) the next ``count`` frames take at most: every JPEG file at its bound ``frame_bytes``, padded"""
        a, b = self.span(count)
        audio = count * 8 + (b - a) * self.writer.bytes_per_sample if self.writer.has_audio else 0
        return count * (8 + int(frame_bytes) + 1) + audio, count * (2 if self.writer.has_audio else 1)

    def make_room(self, count: int, frame_bytes: int, stream_frame: int, check=None) -> None:
        """Before a run of ``count`` frames (the stream's ``stream_frame`` ..) is built: if its worst case no longer fits the file, ask
        ``on_full(sid, which)`` for a fresh writer, whose frame 0 is then ``stream_frame``; AviFull without ``on_full`` (or when the fresh
        file cannot take the run either).  The full writer is the caller's to close."""
        if self.writer.room_for(*self.worst_case(count, frame_bytes)):
            return
        if self.on_full is None:
            raise AviFull("session %d: %d more frames may take the %s file past max_bytes=%d and no on_full was given" % (
                self.sid, count, self.which, self.writer.max_bytes))
        fresh = self.on_full(self.sid, self.which)
        if check is not None:
            check(fresh, self.which)
        self._start(fresh, stream_frame)
        if not self.writer.room_for(*self.worst_case(count, frame_bytes)):
            raise AviFull("session %d: the fresh %s file (max_bytes=%d) cannot take %d frames" % (self.sid, self.which, self.writer.max_bytes, count))


class DeviceMultiMuxer(_MuxBuffers):
    """``lspjpeg_encode`` then ``lspavi_pack_multi`` (include/lspavi.h): one batch of device frames that belongs to up to 16 files becomes
    one fragment per file on the device, with the audio taken from per-session rings.  One encode, two launches, one copy of status + index
    and one copy of the bytes, whatever the number of files.  Uses ``encoder``'s slab like DeviceMuxer."""

    def __init__(self, encoder, rate: int = 16000, fps: int = 60):
        super().__init__(encoder, rate, fps)
        B, N, lib = encoder.max_batch, self.N, self.lib
        self.max_runs = R = min(B, N.AVI_MAX_STREAMS)
        self._srows = R * N.AVI_STATUS_WORDS // 4                                     # rows of 4 words the status rows take
        self._allocate(lib.lspavi_capacity_bytes_multi(len(encoder.header), encoder.capacity, B, R, self.rate, self.fps),
                       lib.lspavi_workspace_bytes_multi(B), self._srows + 2 * B)       # the status rows, then the index
        self._table = (N.AviRun * N.AVI_MAX_STREAMS)()

    def pack(self, frames, runs):
        """``frames``: what JpegEncoder takes; ``runs``: per file, in batch order, ``(count, frame0, audio_format, ring, sample0,
        avail_begin, avail_end)`` -- ``audio_format`` None / "s16" / "f32", ``ring`` that session's contiguous 1-D float32 device tensor.
        -> per run what AviWriter.append_fragment takes; the ``data`` are views of pinned memory, valid until the next pack().  A run the
        ring cannot serve is refused by lspavi_pack_multi on the host (LspaviError): nothing was launched for the mux."""
        import torch
        c = ctypes.c_void_p
        runs = list(runs)
        if not 1 <= len(runs) <= self.N.AVI_MAX_STREAMS:
            raise ValueError("a batch is split into 1..%d runs (got %d)" % (self.N.AVI_MAX_STREAMS, len(runs)))
        first = 0
        for j, (count, frame0, fmt, ring, sample0, begin, end) in enumerate(runs):
            if fmt is not None and not self._is_wave(ring):
                raise ValueError("run %d: the ring must be a contiguous 1-D float32 tensor on %s" % (j, self.device))
            t = self._table[j]
            t.first, t.count, t.audio_format, t.reserved, t.frame0 = first, int(count), self.N.AVI_AUDIO_FORMATS[fmt], 0, int(frame0)
            t.ring_dev = ring.data_ptr() if fmt is not None else None
            t.ring_samples = ring.shape[0] if fmt is not None else 0
            t.sample0, t.avail_begin, t.avail_end = int(sample0), int(begin), int(end)
            first += int(count)
        b = self.enc.enqueue(frames)
        stream = torch.cuda.current_stream(self.device)
        dst, sizes = self.enc.slab
        R = self._srows
        with torch.cuda.device(self.device):
            self.N.check_avi(self.lib.lspavi_pack_multi(
                c(self._header.data_ptr()), len(self.enc.header), c(dst.data_ptr()), self.enc.capacity, c(sizes.data_ptr()), b,
                self._table, len(runs), self.rate, self.fps, c(self._out.data_ptr()), self.capacity,
                c(self._meta[R:].data_ptr()), c(self._meta.data_ptr()), c(self._ws.data_ptr()), self._ws_bytes, c(stream.cuda_stream)))
            self._meta_host[:R + 2 * b].copy_(self._meta[:R + 2 * b], non_blocking=True)
        stream.synchronize()
        meta = self._meta_host.numpy().view(np.uint32)
        status = meta[:R].reshape(-1, self.N.AVI_STATUS_WORDS)[:len(runs)]
        at = row = 0
        for j, (count, frame0, fmt, *_rest) in enumerate(runs):
            off, nbytes, nchunk, _, _, row0 = (int(v) for v in status[j][:6])
            if off != at or row0 != row or nchunk != int(count) * (2 if fmt is not None else 1) or nbytes == 0 or nbytes & 1 \
                    or off + nbytes > self.capacity:
                raise RuntimeError("lspavi_pack_multi: run %d came back as %d bytes at %d in %d chunks from row %d (expected offset %d, row %d)" % (
                    j, nbytes, off, nchunk, row0, at, row))
            at, row = (off + nbytes + 15) & ~15, row + nchunk
        total = int(status[-1][0]) + int(status[-1][1])
        host, out = self._fetch(total, stream), []
        for j, (count, frame0, fmt, *_rest) in enumerate(runs):
            off, nbytes, nchunk, largest_video, largest_audio, row0 = (int(v) for v in status[j][:6])
            nsamples = frame_sample(int(frame0) + int(count), self.rate, self.fps) - frame_sample(frame0, self.rate, self.fps) if fmt is not None else 0
            out.append((host[off:off + nbytes], meta[R + row0:R + row0 + nchunk].copy(), int(count), nsamples, largest_video, largest_audio))
        return out
