"""Audio in, frames out of the same tick: ``LivePortraitPool`` chains the live audio pool, the landmark stage, the rasteriser, the generator
and (optionally) the JPEG encoder on one stream, with nothing on the host in between (DESIGN.md "Landmark stage and live frames").

One avatar per pool: one ``LandmarkStage`` (its constants), one ``Feature2FaceModel`` and one candidate stack, whose share of the first
layers is cached by the engine as in the render loop.  Inside a tick:

1. ``LiveSessionPool.tick``: the audio stages, one call per stage -- mouth rows and head poses of every session, on the device;
2. ``LandmarkStage.tick``: ONE launch -- the points of every frame that became final, of all sessions, in one tensor;
3. ``FeatureMapRasteriser.rasterise_points``: one launch over all those frames;
4. the generator with fused ``tensor2im`` in groups of at most ``max_batch`` frames (``last_groups`` records them);
5. JPEG when asked for.

4b. with ``out_size``: every generator group is resampled once (resize.Resizer: ``Image.resize``, bit for bit) right behind its forward;
   the frames handed out, the JPEG files and the ``video`` recordings are then ``out_size``.  The edge-map recordings stay ``load_size``.

6. recording, for the sessions that have a writer: the frames of a tick are encoded and muxed in groups of at most ``max_batch``, one
   fragment per file out of one ``lspavi_pack_multi`` call, the audio from per-session rings on the device.

0. the audio input stage, for the sessions opened at a capture rate (``open(input_rate=...)``, with a pool built with ``audio_input``):
   ONE launch turns their raw samples (any supported rate, int16 or float32, mono or stereo) into the 16 kHz float32 views that steps 1
   and 6 take exactly as they take device-tensor samples.  Sessions opened without a rate skip it.

The only host copy is the last one, when ``host`` or ``jpeg_quality`` asks for it (and a recorded fragment's bytes).  A frame leaves ``delay`` frames after its audio: the
audio models' lookahead (frame_future, ~18 frames) plus the largest filter radius of the landmark stage (or its ``max_lookahead``)."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple


class LivePortraitPool:
    """``audio``: a LiveSessionPool; ``stage``: a LandmarkStage on the same device with at least as many sessions; ``model``: a
    Feature2FaceModel (set up, eval); ``cand_image``: demo.py's ``img_candidates`` [1, 12, H, W] on the device.  ``max_batch``: frames per
    generator forward.  ``raster_chunk``: frames per rasteriser launch (one launch per tick unless a tick emits more: 1 MiB of map per
    frame).  A tick may bring a session at most ``max_tick_samples`` samples: what the stage's rings (its ``max_push``) can take.

    ``record_quality`` (a JPEG quality or a ``jpeg.JpegOptions``; with its ``subsampling`` set, an ``out_size`` that is no multiple of 16 records as well) makes the pool able to record: it then keeps every session's last ``ring_samples`` samples on the
    device, and ``open`` / ``record`` take AviWriters that ``tick`` appends the session's frames and their audio to.  ``record_route``
    "device" (one lspavi_pack_multi per group of frames) or "host" (JpegEncoder + append_jpegs per session); both write the same files.

    ``audio_input``: an AudioInputStage on the same device with at least as many sessions; sessions may then be opened at one of its rates
    and pushed raw capture audio.  The stage's lookahead (R input samples, at most 8 ms) adds at most one frame to ``delay``.

    ``out_size`` (an int or ``(width, height)``; None: off) with ``resample`` ("box", "bilinear", "hamming", "bicubic", "lanczos"): the colour
    frames leave the pool at that size -- one resize call per generator group, nothing else added to a tick.  ``video`` writers must then be
    of ``out_size``; ``video_input`` (the edge maps, the generator's input) stays ``load_size``."""

    fps = 60                                                                       # live.py: a clip of N samples has int(N / 16000 * 60) frames
    rate = 16000

    def __init__(self, audio, stage, model, cand_image, load_size: int = 512, max_batch: int = 8, raster_chunk: int = 64,
                 record_quality: Optional[int] = None, record_route: Optional[str] = None, audio_input=None, out_size=None,
                 resample: str = "bicubic"):
        import torch
        from .feature_map import FeatureMapRasteriser
        self.torch = torch
        self.audio, self.stage, self.model, self.cand = audio, stage, model, cand_image
        self.device = audio.device
        if (stage.device.index or 0) != (self.device.index or 0):
            raise ValueError("the audio pool and the landmark stage must live on the same device")
        if cand_image.device.type != "cuda" or (cand_image.device.index or 0) != (self.device.index or 0):
            raise ValueError("cand_image must be on the pool's device")
        if stage.max_sessions < audio.max_sessions:
            raise ValueError("the landmark stage has %d sessions, the audio pool %d" % (stage.max_sessions, audio.max_sessions))
        if max_batch < 1 or raster_chunk < 1:
            raise ValueError("max_batch and raster_chunk must be >= 1")
        if audio_input is not None:
            if (audio_input.device.index or 0) != (self.device.index or 0):
                raise ValueError("the audio pool and the audio input stage must live on the same device")
            if audio_input.max_sessions < audio.max_sessions:
                raise ValueError("the audio input stage has %d sessions, the audio pool %d" % (audio_input.max_sessions, audio.max_sessions))
        self.audio_input = audio_input
        self._in: Dict[int, int] = {}                                              # audio session id -> input stage session id
        self.last_heard: Dict[int, tuple] = {}                                     # the input stage's output of the last tick, per session
        self.load_size, self.max_batch, self.raster_chunk = int(load_size), int(max_batch), int(raster_chunk)
        self.raster = FeatureMapRasteriser(self.load_size, 18, self.device)
        self.out_size, self.resample, self._resizer, self._full = None, resample, None, None
        if out_size is not None:
            from .resize import Resizer, check_filter, check_size
            self.out_size, self.resample = check_size(out_size), check_filter(resample)
            self._resizer = Resizer(self.device, max_batch=self.max_batch)
            self._full = torch.empty((self.max_batch, self.load_size, self.load_size, 3), dtype=torch.uint8, device=self.device)     # a group at the generator's size
        self.frame_width, self.frame_height = self.out_size or (self.load_size, self.load_size)                                          # of the colour frames that leave
        rows = stage.max_push - audio.ff_mouth - 2                                # a push's frames, + the mouth tail at finish, + rounding
        if rows < 1:
            raise ValueError("the landmark stage's max_push (%d) must exceed the mouth lookahead + 2 (%d)" % (stage.max_push, audio.ff_mouth + 2))
        self.max_tick_samples = rows * 16000 // 60
        self.delay = max(audio.ff_mouth, audio.ff_head) + max(stage.future)
        self._maps = torch.empty((self.raster_chunk, 1, self.load_size, self.load_size), dtype=torch.float32, device=self.device)
        self._lm: Dict[int, int] = {}                                              # audio session id -> landmark session id
        self._jpeg: Dict[object, object] = {}                                      # jpeg.JpegOptions (the whole option set) -> JpegEncoder
        self.last_groups: List[List[Tuple[int, int]]] = []
        self.last_points = None
        self.record_quality = self.record_route = None
        self._rec: Dict[int, Dict[str, object]] = {}                               # session id -> {"video" / "video_input": LiveRecording}
        self.recording_stopped: Dict[int, Exception] = {}                          # session id -> the AviFull that ended its recording
        if record_quality is None:
            if record_route is not None:
                raise ValueError("record_route needs record_quality")
            return
        from . import video as V
        from .jpeg import JpegOptions
        if isinstance(record_quality, JpegOptions):
            record_quality = JpegOptions.of(record_quality)
        if not 1 <= int(JpegOptions.of(record_quality).quality) <= 100:
            raise ValueError("record_quality must be in 1..100")
        self.record_route = record_route or V.DEFAULT_LIVE_RECORD_ROUTE
        if self.record_route not in ("device", "host"):
            raise ValueError("record_route must be 'device' or 'host'")
        if self.max_batch > 64:
            raise ValueError("a recording pool encodes at most 64 frames per group (max_batch = %d)" % self.max_batch)
        self.record_quality = record_quality if isinstance(record_quality, JpegOptions) else int(record_quality)
        # the oldest frame a tick can emit: delay frames behind the audio, or the landmark filters' full radius while max_lookahead holds the first frames back
        lag = max(audio.ff_mouth, audio.ff_head) + max(stage.radii)
        self.ring_samples = V.live_ring_samples(lag, self.max_tick_samples, self.rate, self.fps)
        self._ring = torch.zeros((audio.max_sessions, self.ring_samples), dtype=torch.float32, device=self.device)
        self._book: Dict[int, object] = {}                                         # session id -> RingBook
        self._emitted: Dict[int, int] = {}                                         # session id -> frames emitted so far
        self._row: Dict[int, int] = {}                                             # session id -> its ring (the audio pool's slot, which it frees at finish)
        self._mux: Dict[str, tuple] = {}                                           # "video" / "video_input" -> (JpegEncoder, DeviceMultiMuxer or None)

    # ---- sessions ----------------------------------------------------------------------------------------------------------------
    def open(self, pre_headpose, generator=None, video=None, video_input=None, on_full=None, input_rate: Optional[int] = None,
             input_format: str = "f32", input_channels: int = 1) -> int:
        """``video`` / ``video_input`` / ``on_full``: record the session from its first frame (see ``record``).  ``input_rate`` (with
        ``input_format`` "f32" / "s16" and ``input_channels`` 1 / 2): the session is pushed raw capture audio of that rate, which the
        pool's ``audio_input`` stage resamples; None: 16 kHz float32 samples, as ever."""
        if input_rate is None:
            if input_format != "f32" or input_channels != 1:
                raise ValueError("input_format and input_channels go with input_rate")
        else:
            if self.audio_input is None:
                raise ValueError("this pool was made without audio_input: it takes 16 kHz float32 samples only")
            self.audio_input.check_spec(input_rate, input_format, input_channels)
        if video is None and (video_input is not None or on_full is not None):
            raise ValueError("video_input and on_full go with video")
        if video is not None:
            self._check_recording(video, video_input)
        sid = self.audio.open(pre_headpose, generator)
        self._lm[sid] = self.stage.open()
        if input_rate is not None:
            self._in[sid] = self.audio_input.open(input_rate, input_format, input_channels)
        if self.record_quality is not None:
            from .video import RingBook
            self._book[sid], self._emitted[sid], self._row[sid] = RingBook(self.ring_samples), 0, self.audio.plan.slot[sid]
            self.recording_stopped.pop(sid, None)
            if video is not None:
                self.record(sid, video, video_input, on_full)
        return sid

    def close(self, sid: int) -> None:
        self.audio.close(sid)
        self.stage.close(self._lm.pop(sid))
        if sid in self._in:
            self.audio_input.close(self._in.pop(sid))
        self._forget(sid)

    def _forget(self, sid: int) -> None:
        self._rec.pop(sid, None)
        if self.record_quality is not None:
            self._book.pop(sid, None)
            self._emitted.pop(sid, None)
            self._row.pop(sid, None)

    # ---- recording ---------------------------------------------------------------------------------------------------------------
    def _check_writer(self, writer, which: str) -> None:
        from .video import AviWriter
        channels = 3 if which == "video" else 1
        if not isinstance(writer, AviWriter) or writer._f is None:
            raise ValueError("%s must be an open AviWriter" % which)
        width, height = (self.frame_width, self.frame_height) if which == "video" else (self.load_size, self.load_size)
        if (writer.width, writer.height, writer.channels, writer.fps) != (width, height, channels, self.fps):
            raise ValueError("%s must be an AviWriter of %dx%d with %d channel(s) at %d fps (got %dx%d, %d, %d fps)" % (
                which, width, height, channels, self.fps, writer.width, writer.height, writer.channels, writer.fps))
        if writer.audio_rate not in (None, self.rate):
            raise ValueError("%s: the audio stream of a live recording is %d Hz (or audio_rate=None), not %d" % (which, self.rate, writer.audio_rate))
        if writer.nframes or writer.nsamples:
            raise ValueError("%s already holds %d frames; a recording starts an empty file" % (which, writer.nframes))

    def _check_recording(self, video, video_input) -> None:
        if self.record_quality is None:
            raise ValueError("this pool was made without record_quality: it cannot record")
        self._check_writer(video, "video")
        if video_input is not None:
            self._check_writer(video_input, "video_input")

    def record(self, sid: int, video, video_input=None, on_full=None) -> None:
        """Record session ``sid`` from its next emitted frame: ``video`` an AviWriter of load_size x load_size x 3 (``out_size`` x 3 with ``out_size``) at the pool's fps,
        with a 16 kHz audio stream or none; ``video_input`` a grayscale one for the rasterised edge maps.  ``on_full(sid, which)`` (which:
        "video" / "video_input") hands out the next writer when a file is full; without it the recording stops there
        (``recording_stopped``).  The writers stay the caller's: ``tick`` appends to them, the caller closes them."""
        from .video import LiveRecording
        if sid not in self._lm:
            self.audio.plan.check(sid)
            raise KeyError("unknown session id %r" % (sid,))
        self._check_recording(video, video_input)
        if sid in self._rec:
            raise ValueError("session %d is being recorded already: stop_recording() first" % sid)
        at = self._emitted[sid]
        self._rec[sid] = {"video": LiveRecording(sid, "video", video, on_full, at)}
        if video_input is not None:
            self._rec[sid]["video_input"] = LiveRecording(sid, "video_input", video_input, on_full, at)
        self.recording_stopped.pop(sid, None)

    def stop_recording(self, sid: int) -> None:
        """no more frames go to the session's writers (the caller closes them)"""
        self._rec.pop(sid, None)

    @property
    def open_sessions(self) -> List[int]:
        return sorted(self._lm)

    # ---- a tick ------------------------------------------------------------------------------------------------------------------
    def tick(self, samples=None, finish=(), host: bool = False, jpeg_quality=None, png=None):
        """Push ``samples`` ({session id: float32 16 kHz samples -- or, for a session opened with ``input_rate``, its raw samples: int16 or
        float32, [n] or [n, channels]}) and end the sessions in ``finish`` (closed afterwards).  -> {id:
        (frame_start, frames)} for every session named: the frames that became final, uint8 [k, H, W, 3] on the device (a numpy array with
        ``host``), or a list of k complete JPEG files (``bytes``) with ``jpeg_quality`` (1..100, or a ``jpeg.JpegOptions``), or of k complete PNG files with ``png`` (True or a ``png.PngOptions``: lossless; not
        together with ``jpeg_quality``).  Nothing is changed when an argument is refused."""
        torch = self.torch
        pairs = list(samples.items()) if hasattr(samples, "items") else list(samples or ())
        finish = list(finish)
        for sid, smp in pairs:
            if sid in self._in:                                                    # the raw count, scaled by M / L
                n16 = -(-len(smp) * 16000 // self.audio_input._sess[self._in[sid]].rate)
                if n16 > self.max_tick_samples:
                    raise ValueError("session %d: %d raw samples (%d at 16 kHz) in one tick; this pool takes at most %d at 16 kHz (the landmark "
                                     "stage's max_push)" % (sid, len(smp), n16, self.max_tick_samples))
            elif len(smp) > self.max_tick_samples:
                raise ValueError("session %d: %d samples in one tick; this pool takes at most %d (the landmark stage's max_push)" % (sid, len(smp), self.max_tick_samples))
        for sid in [s for s, _ in pairs] + finish:
            if sid not in self._lm:
                self.audio.plan.check(sid)                                         # raises what the audio pool raises for a closed / unknown id
                raise KeyError("unknown session id %r" % (sid,))
        if png is not None and png is not False:
            from .png import PngOptions
            png = PngOptions.of(png)
            if jpeg_quality is not None:
                raise ValueError("png and jpeg_quality: a frame leaves as one file, PNG or JPEG")
        else:
            png = None
        if jpeg_quality is not None:
            from .jpeg import JpegOptions
            if isinstance(jpeg_quality, JpegOptions):
                jpeg_quality = JpegOptions.of(jpeg_quality)
            if not 1 <= int(JpegOptions.of(jpeg_quality).quality) <= 100:
                raise ValueError("jpeg_quality must be in 1..100")
        lengths = {sid: len(smp) for sid, smp in pairs}
        staged = [sid for sid in dict.fromkeys([s for s, _ in pairs] + finish) if sid in self._in]
        if staged:
            if len(lengths) != len(pairs):
                raise ValueError("a session appears twice in one tick")
            raw = {self._in[sid]: smp for sid, smp in pairs if sid in self._in}
            fin_in = [self._in[sid] for sid in finish if sid in self._in]
            emits = self.audio_input.preview(raw, fin_in)                          # every check of the input stage, and its 16 kHz counts
            lengths.update({sid: emits[self._in[sid]] for sid in staged})
        self._dry_run(lengths, finish)                                            # the landmark rings take this tick's rows, or nothing runs
        snap, self.last_heard = None, {}
        if staged:                                                                 # 0. one launch: raw capture audio -> 16 kHz views
            snap = self.audio_input.snapshot()
            heard = self.audio_input.tick(raw, finish=fin_in)
            self.last_heard = {sid: heard[self._in[sid]] for sid in staged}       # (first 16 kHz sample, the samples): what the models hear
            pushed = {sid for sid, _ in pairs}
            pairs = [(sid, heard[self._in[sid]][1] if sid in self._in else smp) for sid, smp in pairs]
            pairs += [(sid, heard[self._in[sid]][1]) for sid in staged if sid not in pushed]           # finished without a push: its tail
        try:
            if self.record_quality is not None:
                pairs = self._to_rings(pairs)
            live = self.audio.tick(pairs, finish=finish, host=False)              # 1. mouth rows and poses, on the device
        except Exception:
            if snap is not None:
                self.audio_input.restore(snap)                                     # the audio pool refused an argument: nothing has changed
            raise
        named = sorted(live)
        try:                                                                       # 2. one launch: the points of every final frame
            out = self.stage.tick({self._lm[sid]: live[sid] for sid in named}, finish=[self._lm[sid] for sid in finish])
        except Exception as e:
            raise RuntimeError("the landmark stage refused the rows of this tick after the audio stages had run; the pool cannot continue: %s" % e) from e
        pts = self.last_points = self.stage.last_points
        spans, at = {}, 0
        for sid in named:                                                          # stage.tick lays the sessions out in ascending landmark id == ascending audio id
            start, p = out[self._lm[sid]]
            spans[sid] = (start, at, p.shape[0])
            at += p.shape[0]
        total = at
        assert pts is None or pts.shape[0] == total
        H = self.load_size
        owner = [(sid, spans[sid][0] + i) for sid in named for i in range(spans[sid][2])]
        self.last_groups = []
        recorded = [sid for sid in named if sid in self._rec and spans[sid][2]]
        with torch.cuda.device(self.device):
            frames = torch.empty((total, self.frame_height, self.frame_width, 3), dtype=torch.uint8, device=self.device)
            edges = None
            if any("video_input" in self._rec[sid] for sid in recorded):          # the {0, 255} maps of the same launch, for the gray files
                edges = torch.empty((total, H, H), dtype=torch.uint8, device=self.device)
            for c0 in range(0, total, self.raster_chunk):
                c1 = min(total, c0 + self.raster_chunk)
                maps = self.raster.rasterise_points(pts[c0:c1], out=self._maps[:c1 - c0],            # 3. one launch over the emitted frames
                                                    out_u8=None if edges is None else edges[c0:c1])
                for g0 in range(c0, c1, self.max_batch):                                            # 4. the generator, uint8 HWC out of its last kernel
                    g1 = min(c1, g0 + self.max_batch)
                    if self._resizer is None:
                        self.model.inference_image(maps[g0 - c0:g1 - c0], self.cand, out=frames[g0:g1])
                    else:                                                                           # 4b. the group once, at out_size, into its rows
                        self.model.inference_image(maps[g0 - c0:g1 - c0], self.cand, out=self._full[:g1 - g0])
                        self._resizer.resize(self._full[:g1 - g0], self.out_size, self.resample, out=frames[g0:g1])
                    self.last_groups.append(owner[g0:g1])
            result = {}
            if jpeg_quality is not None or png is not None:                        # 5. complete files; only the compressed bytes cross PCIe
                enc = self._encoder(jpeg_quality) if png is None else self._png_encoder(png)
                files: List[bytes] = []
                for g0 in range(0, total, self.max_batch):
                    files += enc.encode(frames[g0:min(total, g0 + self.max_batch)])
                for sid in named:
                    start, a, n = spans[sid]
                    result[sid] = (start, files[a:a + n])
            else:
                data = frames.cpu().numpy() if host else frames                    # one copy, whatever the number of sessions
                for sid in named:
                    start, a, n = spans[sid]
                    result[sid] = (start, data[a:a + n])
            if recorded:                                                           # 6. the recorded sessions' frames, into their files
                self._record_track("video", [(sid,) + spans[sid] for sid in recorded], frames)
                self._record_track("video_input", [(sid,) + spans[sid] for sid in recorded], edges)
        if self.record_quality is not None:
            for sid in named:
                self._emitted[sid] += spans[sid][2]
        for sid in finish:
            del self._lm[sid]
            self._in.pop(sid, None)                                                # the input stage closed it in its own tick
            self._forget(sid)
        return result

    def _to_rings(self, pairs):
        """This tick's samples as ONE device tensor (one upload for all host arrays), appended to the sessions' rings in one index_copy_
        whether or not a session is being recorded; -> the pairs with device views, which LiveSessionPool.tick takes as they are."""
        import numpy as np
        torch = self.torch
        out, parts, at = [], [], []
        host = [(sid, np.asarray(smp)) for sid, smp in pairs if not isinstance(smp, torch.Tensor)]
        bad = [sid for sid, a in host if a.dtype != np.float32 or a.ndim != 1]
        bad += [sid for sid, t in pairs if isinstance(t, torch.Tensor) and (t.dtype != torch.float32 or t.dim() != 1)]
        if bad or len({sid for sid, _ in pairs}) != len(pairs):
            return pairs                                                           # the audio pool refuses these, with its own words
        with torch.cuda.device(self.device):
            flat = torch.from_numpy(np.ascontiguousarray(np.concatenate([a for _, a in host]))).to(self.device) if host else None
            off = 0
            for sid, smp in pairs:
                if isinstance(smp, torch.Tensor):
                    t = smp.to(self.device).contiguous()
                else:
                    t = flat[off:off + len(smp)]
                    off += len(smp)
                out.append((sid, t))
                if t.shape[0]:
                    parts.append(t)
                    at.append(self._row[sid] * self.ring_samples + self._book[sid].push(t.shape[0]))
            if parts:
                self._ring.view(-1).index_copy_(0, torch.from_numpy(np.concatenate(at)).to(self.device), parts[0] if len(parts) == 1 else torch.cat(parts))
        return out

    def _track(self, which: str):
        pair = self._mux.get(which)
        if pair is None:
            from .jpeg import JpegEncoder
            from .video import DeviceMultiMuxer
            size = (self.frame_height, self.frame_width) if which == "video" else self.load_size
            enc = JpegEncoder(size, 3 if which == "video" else 1, self.record_quality, self.device, max_batch=self.max_batch)
            pair = self._mux[which] = (enc, DeviceMultiMuxer(enc, self.rate, self.fps) if self.record_route == "device" else None)
        return pair

    def _record_track(self, which: str, segments, source) -> None:
        """``segments``: (sid, first stream frame, first row of ``source``, count) of the recorded sessions, ascending.  Groups of at most
        ``max_batch`` frames; a group is made of runs, one per file; a session may span two groups.  Before a run is taken into a group its
        file is asked for room (LiveRecording.make_room): rollover, or the end of that session's recording."""
        from .video import AviFull
        queue = [list(s) for s in segments if which in self._rec.get(s[0], ())]
        if not queue:
            return
        enc, mux = self._track(which)
        frame_bytes = len(enc.header) + enc.capacity
        while queue:
            group, room = [], self.max_batch
            while queue and room:
                sid, start, row, n = queue[0]
                if sid not in self._rec:                                           # stopped while its other file was written
                    queue.pop(0)
                    continue
                rec, take = self._rec[sid][which], min(n, room)
                try:
                    rec.make_room(take, frame_bytes, start, self._check_writer)
                except AviFull as e:
                    self.recording_stopped[sid] = e
                    del self._rec[sid]
                    queue.pop(0)
                    continue
                if rec.base + rec.writer.nframes != start:
                    raise RuntimeError("session %d: frame %d follows %d recorded frames from %d" % (sid, start, rec.writer.nframes, rec.base))
                group.append((sid, rec, row, take))
                room -= take
                if take == n:
                    queue.pop(0)
                else:
                    queue[0] = [sid, start + take, row + take, n - take]
            if group:
                self._record_group(enc, mux, group, source)

    def _record_group(self, enc, mux, group, source) -> None:
        torch = self.torch
        if all(a[2] + a[3] == b[2] for a, b in zip(group, group[1:])):            # consecutive in ``source``: no copy
            frames = source[group[0][2]:group[-1][2] + group[-1][3]]
        else:                                                                      # an unrecorded session's frames lie in between
            frames = torch.cat([source[row:row + n] for _, _, row, n in group])
        runs = []
        for sid, rec, row, n in group:
            fmt = rec.writer.audio_format
            a, b = self._book[sid].avail
            runs.append((n, rec.writer.nframes, fmt, self._ring[self._row[sid]] if fmt else None, rec.sample0, a, b))
        if mux is not None:
            for (sid, rec, _, _), fragment in zip(group, mux.pack(frames, runs)):
                rec.writer.append_fragment(*fragment)
            return
        files, at = enc.encode(frames), 0
        for sid, rec, _, n in group:
            samples = None
            if rec.writer.has_audio:
                pos = self._book[sid].positions(*rec.span(n))
                samples = self._ring[self._row[sid]][torch.from_numpy(pos).to(self.device)].cpu().numpy()
            rec.writer.append_jpegs(files[at:at + n], samples)
            at += n

    def _dry_run(self, lengths, finish) -> None:
        """How many mouth rows and poses the audio stages will hand over is host arithmetic (PoolPlanner.preview): push the counts through
        copies of the landmark schedulers, so that a tick the rings cannot take is refused before any stage has run."""
        import copy
        for sid, (mouth, poses) in self.audio.plan.preview(lengths, set(finish)).items():
            copy.copy(self.stage.sched[self._lm[sid]]).push(mouth, poses, sid in finish)

    def _encoder(self, quality):
        from .jpeg import JpegOptions
        quality = JpegOptions.of(quality)                                          # 75 and JpegOptions(75) are one encoder
        enc = self._jpeg.get(quality)
        if enc is None:
            from .jpeg import JpegEncoder
            enc = self._jpeg[quality] = JpegEncoder((self.frame_height, self.frame_width), 3, quality, self.device, max_batch=self.max_batch)
        return enc

    def _png_encoder(self, options):
        enc = self._jpeg.get(("png", options))                                     # (one table of encoders; a JpegOptions is no such pair)
        if enc is None:
            from .png import PngEncoder
            enc = self._jpeg[("png", options)] = PngEncoder((self.frame_height, self.frame_width), 3, self.device, max_batch=self.max_batch, level=options)
        return enc
