"""Audio in, frames out of the same tick: ``LivePortraitPool`` chains the live audio pool, the landmark stage, the rasteriser, the generator
and (optionally) the JPEG encoder on one stream, with nothing on the host in between (DESIGN.md "Landmark stage and live frames").

One avatar per pool: one ``LandmarkStage`` (its constants), one ``Feature2FaceModel`` and one candidate stack, whose share of the first
layers is cached by the engine as in the render loop.  Inside a tick:

1. ``LiveSessionPool.tick``: the audio stages, one call per stage -- mouth rows and head poses of every session, on the device;
2. ``LandmarkStage.tick``: ONE launch -- the points of every frame that became final, of all sessions, in one tensor;
3. ``FeatureMapRasteriser.rasterise_points``: one launch over all those frames;
4. the generator with fused ``tensor2im`` in groups of at most ``max_batch`` frames (``last_groups`` records them);
5. JPEG when asked for.

The only host copy is the last one, when ``host`` or ``jpeg_quality`` asks for it.  A frame leaves ``delay`` frames after its audio: the
audio models' lookahead (frame_future, ~18 frames) plus the largest filter radius of the landmark stage (or its ``max_lookahead``)."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple


class LivePortraitPool:
    """``audio``: a LiveSessionPool; ``stage``: a LandmarkStage on the same device with at least as many sessions; ``model``: a
    Feature2FaceModel (set up, eval); ``cand_image``: demo.py's ``img_candidates`` [1, 12, H, W] on the device.  ``max_batch``: frames per
    generator forward.  ``raster_chunk``: frames per rasteriser launch (one launch per tick unless a tick emits more: 1 MiB of map per
    frame).  A tick may bring a session at most ``max_tick_samples`` samples: what the stage's rings (its ``max_push``) can take."""

    def __init__(self, audio, stage, model, cand_image, load_size: int = 512, max_batch: int = 8, raster_chunk: int = 64):
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
        self.load_size, self.max_batch, self.raster_chunk = int(load_size), int(max_batch), int(raster_chunk)
        self.raster = FeatureMapRasteriser(self.load_size, 18, self.device)
        rows = stage.max_push - audio.ff_mouth - 2                                # a push's frames, + the mouth tail at finish, + rounding
        if rows < 1:
            raise ValueError("the landmark stage's max_push (%d) must exceed the mouth lookahead + 2 (%d)" % (stage.max_push, audio.ff_mouth + 2))
        self.max_tick_samples = rows * 16000 // 60
        self.delay = max(audio.ff_mouth, audio.ff_head) + max(stage.future)
        self._maps = torch.empty((self.raster_chunk, 1, self.load_size, self.load_size), dtype=torch.float32, device=self.device)
        self._lm: Dict[int, int] = {}                                              # audio session id -> landmark session id
        self._jpeg: Dict[int, object] = {}                                         # quality -> JpegEncoder
        self.last_groups: List[List[Tuple[int, int]]] = []
        self.last_points = None

    # ---- sessions ----------------------------------------------------------------------------------------------------------------
    def open(self, pre_headpose, generator=None) -> int:
        sid = self.audio.open(pre_headpose, generator)
        self._lm[sid] = self.stage.open()
        return sid

    def close(self, sid: int) -> None:
        self.audio.close(sid)
        self.stage.close(self._lm.pop(sid))

    @property
    def open_sessions(self) -> List[int]:
        return sorted(self._lm)

    # ---- a tick ------------------------------------------------------------------------------------------------------------------
    def tick(self, samples=None, finish=(), host: bool = False, jpeg_quality: Optional[int] = None):
        """Push ``samples`` ({session id: float32 16 kHz samples}) and end the sessions in ``finish`` (closed afterwards).  -> {id:
        (frame_start, frames)} for every session named: the frames that became final, uint8 [k, H, W, 3] on the device (a numpy array with
        ``host``), or a list of k complete JPEG files (``bytes``) with ``jpeg_quality``.  Nothing is changed when an argument is refused."""
        torch = self.torch
        pairs = list(samples.items()) if hasattr(samples, "items") else list(samples or ())
        finish = list(finish)
        for sid, smp in pairs:
            if len(smp) > self.max_tick_samples:
                raise ValueError("session %d: %d samples in one tick; this pool takes at most %d (the landmark stage's max_push)" % (sid, len(smp), self.max_tick_samples))
        for sid in [s for s, _ in pairs] + finish:
            if sid not in self._lm:
                self.audio.plan.check(sid)                                         # raises what the audio pool raises for a closed / unknown id
                raise KeyError("unknown session id %r" % (sid,))
        if jpeg_quality is not None and not 1 <= int(jpeg_quality) <= 100:
            raise ValueError("jpeg_quality must be in 1..100")
        self._dry_run({sid: len(smp) for sid, smp in pairs}, finish)              # the landmark rings take this tick's rows, or nothing runs
        live = self.audio.tick(pairs, finish=finish, host=False)                  # 1. mouth rows and poses, on the device
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
        with torch.cuda.device(self.device):
            frames = torch.empty((total, H, H, 3), dtype=torch.uint8, device=self.device)
            for c0 in range(0, total, self.raster_chunk):
                c1 = min(total, c0 + self.raster_chunk)
                maps = self.raster.rasterise_points(pts[c0:c1], out=self._maps[:c1 - c0])            # 3. one launch over the emitted frames
                for g0 in range(c0, c1, self.max_batch):                                            # 4. the generator, uint8 HWC out of its last kernel
                    g1 = min(c1, g0 + self.max_batch)
                    self.model.inference_image(maps[g0 - c0:g1 - c0], self.cand, out=frames[g0:g1])
                    self.last_groups.append(owner[g0:g1])
            result = {}
            if jpeg_quality is not None:                                           # 5. complete files; only the compressed bytes cross PCIe
                enc = self._encoder(int(jpeg_quality))
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
        for sid in finish:
            del self._lm[sid]
        return result

    def _dry_run(self, lengths, finish) -> None:
        """How many mouth rows and poses the audio stages will hand over is host arithmetic (PoolPlanner.preview): push the counts through
        copies of the landmark schedulers, so that a tick the rings cannot take is refused before any stage has run."""
        import copy
        for sid, (mouth, poses) in self.audio.plan.preview(lengths, set(finish)).items():
            copy.copy(self.stage.sched[self._lm[sid]]).push(mouth, poses, sid in finish)

    def _encoder(self, quality: int):
        enc = self._jpeg.get(quality)
        if enc is None:
            from .jpeg import JpegEncoder
            enc = self._jpeg[quality] = JpegEncoder(self.load_size, 3, quality, self.device, max_batch=self.max_batch)
        return enc
