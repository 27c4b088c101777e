"""The audio input stage: demo.py:179 (``audio, _ = librosa.load(opt.driving_audio, sr=sr)``) on the device (include/lsprs.h,
csrc/resample.hip).

Raw capture audio -- 8 .. 192 kHz, float32 or int16, one or two interleaved channels -- in, the 16 kHz mono float32 signal of every other
stage out.  ``AudioInputStage`` is the streamed, pooled form for up to 16 sessions of up to 4 rates: ONE launch per tick whatever the
number of sessions, no device-to-host read -- every count comes from ``ResampleScheduler``, which needs no device.  ``resample_clip`` is
the whole-clip form and ``load_audio`` reads a RIFF/WAVE file into it.  A stream pushed in pieces equals the stream pushed at once, bit
for bit: both run the same device function per output.

PARITY-UNPINNED against librosa: librosa 0.7 resamples through resampy's ``kaiser_best``, a 512-per-zero-crossing table of a Kaiser
windowed sinc read with linear interpolation.  This stage computes the ideal filter that table approximates, in closed form (lsprs.h
states it; tests/resample_model.py restates it in float64), and emits all ``ceil(N * 16000 / rate)`` samples where resampy stops one short
and librosa pads a zero.  tools/pin_resample_fixture.py records librosa's own output where librosa is installed.

16 kHz mono float32 is a passthrough: the input bits, no launch.  Other 16 kHz input is converted and downmixed but not filtered
(librosa.load does not resample at the target rate either).  There is no CPU path."""
from __future__ import annotations

import ctypes
import math
import struct
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np

OUT_RATE = 16000
ZEROS = 64                                      # resampy's kaiser_best
MAX_SESSIONS = 16
MAX_RATES = 4
FORMATS = ("f32", "s16")


def ratio(rate: int) -> Tuple[int, int, int]:
    """(L, M, R) of an input rate: 16000 / rate = L / M in lowest terms, R = ceil(64 / min(1, L / M)) the filter's half-width in input
    samples (0 at 16 kHz: no filter)."""
    rate = int(rate)
    g = math.gcd(rate, OUT_RATE)
    L, M = OUT_RATE // g, rate // g
    R = 0 if rate == OUT_RATE else (-(-ZEROS * M // L) if M > L else ZEROS)
    return L, M, R


def final_outputs(rate: int, n_in: int, finished: bool) -> int:
    """How many outputs of a stream of ``n_in`` input samples are final (lsprs_out_count): while the stream runs, output j is final when
    its last tap is present, (j M) div L + R <= n_in - 1; at finish all ceil(n_in L / M) are."""
    L, M, R = ratio(rate)
    m = n_in if finished else n_in - R
    return 0 if m <= 0 else -(-m * L // M)


class ResamplePlan(NamedTuple):
    """What one push of one session does (the counts of lsprs_session_call)."""
    n_have: int
    n_fresh: int
    out0: int
    n_out: int
    finished: bool


class ResampleScheduler:
    """When an output sample becomes final, without a device (``final_outputs``).  ``lookahead_samples`` = R input samples: 4 ms at any
    rate >= 16 kHz, 8 ms at 8 kHz."""

    def __init__(self, rate: int, max_push: int):
        self.rate, self.max_push = int(rate), int(max_push)
        self.L, self.M, self.R = ratio(rate)
        self.n = self.e = 0                                                        # input samples taken, outputs emitted
        self.ended = False

    @property
    def lookahead_samples(self) -> int:
        return self.R

    def push(self, n_fresh: int, finish: bool = False) -> ResamplePlan:
        if self.ended:
            raise RuntimeError("the session has finished")
        if n_fresh < 0:
            raise ValueError("negative sample count")
        if n_fresh > self.max_push:
            raise ValueError("%d samples in one tick; the input stage's rings take at most %d (its max_push)" % (n_fresh, self.max_push))
        n = self.n + n_fresh
        end = final_outputs(self.rate, n, finish)
        plan = ResamplePlan(self.n, n_fresh, self.e, end - self.e, bool(finish))
        self.n, self.e, self.ended = n, end, bool(finish)
        return plan


class _Session(NamedTuple):
    slot: int
    rate: int
    fmt: str
    channels: int
    sched: ResampleScheduler


def _spec(rate, fmt, channels, rates) -> None:
    if fmt not in FORMATS:
        raise ValueError("input format must be one of %s (got %r)" % (FORMATS, fmt))
    if channels not in (1, 2):
        raise ValueError("%r channels: one or two interleaved channels are supported" % (channels,))
    if int(rate) not in rates and not (int(rate) == OUT_RATE and fmt == "f32" and channels == 1):
        raise ValueError("rate %r is not one of this stage's rates %s" % (rate, tuple(rates)))


class AudioInputStage:
    """``rates``: up to 4 input rates (16000 needs no entry unless it comes as int16 or stereo).  ``max_push``: the most input samples
    (per channel) one session brings in one tick.  Sessions: ``open`` / ``tick`` / ``close``; whole clips: ``resample_clip``."""

    def __init__(self, rates: Sequence[int], device="cuda:0", max_sessions: int = MAX_SESSIONS, max_push: int = 9600):
        import torch
        from . import _native as N
        self.torch, self.N = torch, N
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("the audio input stage runs on the MI355X only (no CPU path); the reference's host path is librosa.load (demo.py:179)")
        rates = [int(r) for r in rates]
        if OUT_RATE not in rates and len(rates) < MAX_RATES:
            rates.append(OUT_RATE)                                                 # int16 / stereo input at 16 kHz: conversion only
        self.device, self.rates = dev, tuple(rates)
        self.max_sessions, self.max_push = int(max_sessions), int(max_push)
        self.lib = N.load()
        cfg = N.RsConfig(abi_version=N.RS_ABI_VERSION, n_rates=len(rates), max_sessions=self.max_sessions, max_push=self.max_push)
        if len(rates) > MAX_RATES:
            raise ValueError("an input stage serves at most %d rates (got %s)" % (MAX_RATES, rates))
        for i, r in enumerate(rates):
            cfg.rates[i] = r
        self.h = ctypes.c_void_p()
        N.check_rs(self.lib.lsprs_create(ctypes.byref(cfg), ctypes.byref(self.h)))
        nbytes = int(self.lib.lsprs_params_bytes(self.h))
        host = np.zeros(nbytes, np.uint8)
        N.check_rs(self.lib.lsprs_pack_params(self.h, host.ctypes.data, nbytes))
        self.history = int(self.lib.lsprs_history(self.h))
        with torch.cuda.device(dev):
            self._params = torch.from_numpy(host).to(dev)                          # uploaded once
            self._state = torch.zeros(int(self.lib.lsprs_state_bytes(self.h)) // 4, dtype=torch.float32, device=dev)
        N.check_rs(self.lib.lsprs_bind_params(self.h, ctypes.c_void_p(self._params.data_ptr()), nbytes))
        N.check_rs(self.lib.lsprs_bind_state(self.h, ctypes.c_void_p(self._state.data_ptr()), self._state.numel() * 4))
        self._free = list(range(self.max_sessions))
        self._sess: Dict[int, _Session] = {}
        self._next = 0

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            self.lib.lsprs_destroy(h)

    @property
    def launches(self) -> int:
        """kernel launches this stage has enqueued so far (the library's own counter)"""
        return int(self.lib.lsprs_launch_count(self.h))

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    # ---- sessions ----------------------------------------------------------------------------------------------------------------
    def check_spec(self, rate: int, fmt: str = "f32", channels: int = 1) -> None:
        _spec(rate, fmt, channels, self.rates)

    def open(self, rate: int, fmt: str = "f32", channels: int = 1) -> int:
        """A new session in a free ring slot -> its id (never reused; the slot is)."""
        self.check_spec(rate, fmt, channels)
        if not self._free:
            raise RuntimeError("all %d sessions of the input stage are open: close one first" % self.max_sessions)
        sid, self._next = self._next, self._next + 1
        self._sess[sid] = _Session(self._free.pop(0), int(rate), fmt, int(channels), ResampleScheduler(rate, self.max_push))
        return sid

    def close(self, sid: int) -> None:
        self._check(sid)
        self._free.append(self._sess.pop(sid).slot)
        self._free.sort()

    def _check(self, sid) -> None:
        if sid not in self._sess:
            raise KeyError("unknown or closed input session %r" % (sid,))

    @property
    def open_sessions(self):
        return sorted(self._sess)

    def lookahead_samples(self, sid: int) -> int:
        self._check(sid)
        return self._sess[sid].sched.R

    def passthrough(self, sid: int) -> bool:
        s = self._sess[sid]
        return s.rate == OUT_RATE and s.fmt == "f32" and s.channels == 1

    def _raw(self, raw, fmt: str, channels: int, who: str):
        """a host array or a device tensor of the session's format: [n] (one channel) or [n, channels] -> (array or tensor, n)"""
        torch = self.torch
        want = {"f32": (np.float32, torch.float32), "s16": (np.int16, torch.int16)}[fmt]
        if isinstance(raw, torch.Tensor):
            dtype, shape = raw.dtype, tuple(raw.shape)
            ok = dtype == want[1]
        else:
            raw = np.asarray(raw)
            dtype, shape = raw.dtype, raw.shape
            ok = dtype == want[0]
        if not ok or not ((len(shape) == 1 and channels == 1) or (len(shape) == 2 and shape[1] == channels)):
            raise ValueError("%s: samples must be %s [n%s] (got %s %s)" % (who, fmt, "" if channels == 1 else ", %d" % channels, dtype, shape))
        return raw, int(shape[0])

    def _upload(self, items):
        """``items``: host arrays and device tensors -> device tensors; all host arrays go up in ONE copy (16-byte aligned pieces)"""
        torch = self.torch
        host = [(i, np.ascontiguousarray(a)) for i, a in enumerate(items) if not isinstance(a, torch.Tensor) and a.size]
        out = list(items)
        offs, total = [], 0
        for _, a in host:
            offs.append(total)
            total += (a.nbytes + 15) & ~15
        if host:
            buf = np.zeros(total, np.uint8)
            for (_, a), o in zip(host, offs):
                buf[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
            flat = torch.from_numpy(buf).to(self.device)
            for (i, a), o in zip(host, offs):
                out[i] = flat[o:o + a.nbytes].view(torch.float32 if a.dtype == np.float32 else torch.int16).view(a.shape)
        for i, a in enumerate(out):
            if isinstance(a, torch.Tensor):
                out[i] = a.to(self.device).contiguous()
            else:                                                                  # an empty host array
                out[i] = torch.empty(a.shape, dtype=torch.float32 if a.dtype == np.float32 else torch.int16, device=self.device)
        return out

    def preview(self, raw, finish=()) -> Dict[int, int]:
        """The argument checks of ``tick`` alone -> {id: how many 16 kHz samples that tick would emit}; changes nothing."""
        return {sid: n_out for sid, (_, _, n_out) in self._plan(raw, finish)[0].items()}

    def _plan(self, raw, finish):
        pairs = list(raw.items()) if hasattr(raw, "items") else list(raw or ())
        finish = list(finish)
        given = {}
        for sid, a in pairs:
            if sid in given:
                raise ValueError("input session %d appears twice in one tick" % sid)
            self._check(sid)
            s = self._sess[sid]
            given[sid] = self._raw(a, s.fmt, s.channels, "input session %d" % sid)
        if len(set(finish)) != len(finish):
            raise ValueError("a session appears twice in finish")
        for sid in finish:
            self._check(sid)
        plans = {}
        for sid in sorted(set(given) | set(finish)):
            sch = self._sess[sid].sched
            if sch.ended:
                raise RuntimeError("input session %d has finished" % sid)
            n = given[sid][1] if sid in given else 0
            if n > self.max_push:
                raise ValueError("input session %d: %d samples in one tick; the stage's rings take at most %d (max_push)" % (sid, n, self.max_push))
            end = final_outputs(sch.rate, sch.n + n, sid in finish)
            plans[sid] = (given[sid][0] if sid in given else None, n, end - sch.e)
        return plans, finish

    def tick(self, raw=None, finish=()):
        """``raw``: {session id: samples} -- a host array or a device tensor, int16 or float32 as the session was opened, [n] or
        [n, channels]; ``finish``: sessions that end after them (closed afterwards).  -> {id: (first_output_index, float32 device tensor)}
        for every session named: the 16 kHz samples that became final.  One launch; all host arrays go up in one copy; nothing is read
        back.  Nothing is changed when an argument is refused."""
        torch = self.torch
        plans, finish = self._plan(raw, finish)
        named = sorted(plans)
        with torch.cuda.device(self.device):
            dev = dict(zip(named, self._upload([plans[sid][0] if plans[sid][0] is not None else np.zeros(0, np.float32) for sid in named])))
            run = [sid for sid in named if not self.passthrough(sid)]
            out = torch.empty(sum(plans[sid][2] for sid in run), dtype=torch.float32, device=self.device)
            calls = (self.N.RsSessionCall * max(len(run), 1))()
            result, at = {}, 0
            for i, sid in enumerate(run):
                s, (_, n, n_out) = self._sess[sid], plans[sid]
                o = out[at:at + n_out]
                at += n_out
                c = calls[i]
                c.slot, c.rate_index, c.format, c.channels = s.slot, self.rates.index(s.rate), self.N.RS_FORMATS[s.fmt], s.channels
                c.n_have, c.out0, c.n_fresh, c.n_out, c.finished = s.sched.n, s.sched.e, n, n_out, int(sid in finish)
                c.fresh_dev = dev[sid].data_ptr() if n else None
                c.out_dev = o.data_ptr() if n_out else None
                result[sid] = (s.sched.e, o)
            if run:
                self.N.check_rs(self.lib.lsprs_tick(self.h, len(run), calls, self._stream()))      # refused: nothing was enqueued, nothing changed
            for sid in named:
                if sid not in result:                                              # 16 kHz mono float32: the input bits
                    result[sid] = (self._sess[sid].sched.e, dev[sid].reshape(-1))
        for sid in named:
            self._sess[sid].sched.push(plans[sid][1], sid in finish)
        for sid in finish:
            self.close(sid)
        return result

    def finish(self, sid: int):
        """End a session without new samples -> (first_output_index, samples) of the tail."""
        return self.tick({}, finish=[sid])[sid]

    def snapshot(self):
        """the host state (slots and counts); ``restore`` makes a tick undone -- the ring slots a tick wrote are none that an earlier state reads"""
        return (list(self._free), {sid: (s, s.sched.n, s.sched.e, s.sched.ended) for sid, s in self._sess.items()}, self._next)

    def restore(self, snap) -> None:
        free, sess, nxt = snap
        self._free, self._next, self._sess = list(free), nxt, {}
        for sid, (s, n, e, ended) in sess.items():
            s.sched.n, s.sched.e, s.sched.ended = n, e, ended
            self._sess[sid] = s

    # ---- whole clip --------------------------------------------------------------------------------------------------------------
    def resample_clip(self, raw, rate: int, fmt: Optional[str] = None, channels: Optional[int] = None):
        """All ``ceil(n * 16000 / rate)`` output samples of a clip -> float32 device tensor.  ``fmt`` / ``channels`` default to what the
        array says (int16 -> "s16", [n, 2] -> 2)."""
        torch = self.torch
        if fmt is None:
            fmt = "s16" if raw.dtype in (np.int16, torch.int16) else "f32"
        if channels is None:
            channels = int(raw.shape[1]) if len(raw.shape) == 2 else 1
        self.check_spec(rate, fmt, channels)
        raw, n = self._raw(raw, fmt, channels, "clip")
        with torch.cuda.device(self.device):
            x = self._upload([raw])[0]
            if int(rate) == OUT_RATE and fmt == "f32" and channels == 1:
                return x.reshape(-1)
            k = self.rates.index(int(rate))
            n_out = final_outputs(rate, n, True)
            out = torch.empty(n_out, dtype=torch.float32, device=self.device)
            ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
            self.N.check_rs(self.lib.lsprs_clip(self.h, k, self.N.RS_FORMATS[fmt], channels, ptr(x), n, ptr(out), n_out, self._stream()))
        return out


# ---- RIFF / WAVE --------------------------------------------------------------------------------------------------------------------
_PCM, _FLOAT, _EXTENSIBLE = 1, 3, 0xFFFE


def read_wav(path) -> Tuple[np.ndarray, int]:
    """A RIFF/WAVE file -> (samples, rate): int16 for format 1 with 16-bit samples, float32 for format 3 with 32-bit samples (the
    reference's driving clip, which the standard library's ``wave`` refuses), WAVE_FORMAT_EXTENSIBLE wrapping either; [n] for one channel,
    [n, 2] for two; chunks in any order, odd-sized chunks padded.  Anything else raises a ValueError that names what was found."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("%s: not a RIFF/WAVE file (it starts with %r)" % (path, data[:12]))
    fmt = body = None
    at = 12
    while at + 8 <= len(data):
        tag, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        if at + 8 + size > len(data):
            raise ValueError("%s: truncated: chunk %r at byte %d claims %d bytes, %d are left" % (path, tag, at, size, len(data) - at - 8))
        if tag == b"fmt " and fmt is None:
            fmt = data[at + 8:at + 8 + size]
        elif tag == b"data" and body is None:
            body = data[at + 8:at + 8 + size]
        at += 8 + size + (size & 1)
    if fmt is None or body is None:
        raise ValueError("%s: no %s chunk" % (path, "'fmt '" if fmt is None else "'data'"))
    if len(fmt) < 16:
        raise ValueError("%s: a 'fmt ' chunk of %d bytes" % (path, len(fmt)))
    tag, channels, rate, _, align, bits = struct.unpack_from("<HHIIHH", fmt, 0)
    if tag == _EXTENSIBLE:
        if len(fmt) < 40:
            raise ValueError("%s: WAVE_FORMAT_EXTENSIBLE with a 'fmt ' chunk of %d bytes" % (path, len(fmt)))
        tag = struct.unpack_from("<H", fmt, 24)[0]                                  # the first two bytes of the SubFormat GUID
    if channels not in (1, 2):
        raise ValueError("%s: %d channels (1 or 2 are supported)" % (path, channels))
    if (tag, bits) == (_PCM, 16):
        dtype = np.dtype("<i2")
    elif (tag, bits) == (_FLOAT, 32):
        dtype = np.dtype("<f4")
    else:
        raise ValueError("%s: WAVE format %d with %d-bit samples (format 1 with 16 bits and format 3 with 32 bits are supported)" % (path, tag, bits))
    frame = dtype.itemsize * channels
    if len(body) % frame:
        raise ValueError("%s: truncated: %d data bytes are no multiple of the %d-byte frame" % (path, len(body), frame))
    a = np.frombuffer(body, dtype).astype(dtype.newbyteorder("="), copy=True)
    return (a if channels == 1 else a.reshape(-1, 2)), int(rate)


def load_audio(path, sr: int = OUT_RATE, device="cuda:0", stage: Optional[AudioInputStage] = None):
    """``librosa.load(path, sr=16000)`` of demo.py:179 for RIFF/WAVE files -> 16 kHz mono float32 tensor on ``device``.  A 16 kHz mono
    float32 file (the reference's clip) comes back bit for bit, without a launch; everything else goes through ``resample_clip`` of
    ``stage`` (made here for the file's rate when None)."""
    import torch
    if int(sr) != OUT_RATE:
        raise ValueError("the pipeline runs at %d Hz; sr=%r is not supported" % (OUT_RATE, sr))
    samples, rate = read_wav(path)
    if rate == OUT_RATE and samples.dtype == np.float32 and samples.ndim == 1:
        return torch.from_numpy(samples).to(device)
    if stage is None:
        stage = AudioInputStage([rate], device, max_sessions=1)
    return stage.resample_clip(samples, rate)
