"""Batched render loop -- the demo.py:260-272 frame loop restated for throughput.

The reference renders one frame per ``inference()`` call (batch 1) and converts each result on the CPU
(``util.tensor2im``, demo.py:268).  The generator is stateless across frames, so the same loop can feed B
feature maps per call, share the constant candidate stack (cand batch 1), take uint8 HWC frames straight
from the last kernel and overlap the D2H copy of batch i with the rendering of batch i+1.
"""
from __future__ import annotations

import inspect
from typing import Callable, Iterable, Iterator, List, Optional

import numpy as np
import torch


def batched(it: Iterable, n: int) -> Iterator[List]:
    buf: List = []
    for x in it:
        buf.append(x)
        if len(buf) == n:
            yield buf
            buf = []
    if buf:
        yield buf


def render_frames(model, feature_maps: Iterable[torch.Tensor], cand_image: torch.Tensor, batch: int = 8,
                  device: Optional[torch.device] = None,
                  on_frame: Optional[Callable[[int, np.ndarray], None]] = None, streams: int = 2,
                  jpeg_quality=None, video=None, audio=None, video_route: Optional[str] = None,
                  out_size=None, resample: str = "bicubic", png=None) -> List[np.ndarray]:
    """``feature_maps`` yields [1,H,W] (or [C,H,W]) CPU/GPU tensors as
    ``facedataset.dataset.get_data_test_mode`` does (demo.py:262); ``cand_image`` is demo.py's
    ``img_candidates`` ([1,12,H,W], already on the device).  Returns (or streams to ``on_frame``) uint8 HWC
    frames, i.e. exactly what ``util.tensor2im(pred_fake[0])`` produced per frame in the reference loop.
    ``model`` is a Feature2FaceModel (anything with ``inference_image``).

    ``streams`` lanes, each a HIP stream, a handle on the same packed weights (``inference_image(replica=k)``) and its own buffers (pinned staging tensor for the maps, their
    device tensor, the frames' device tensor, a pinned tensor for the frames): batch n runs on lane n % streams; before a lane is reused the host waits for THAT STREAM to drain
    and hands out its frames.  Nothing is allocated per batch, the maps of the next batch are gathered
    into pinned memory while the lanes render, and two batches in flight fill each other's kernel tails (generator alone: +5 % at 8 fp32 frames, +16 % on the 16-bit plans).
    Measured, round 5 (tools/render_loop_profile.py, tools/host_probe.py): the loop of rounds 2-4 ran at 70-290 frames/s on a generator that renders 665-1019 -- because of the
    host-side copy described at the gather below, not because of how it waited or allocated (a hipGraph cache miss costs nothing next to a forward; the late event waits seen in the
    first measurements were not separated from that throttling).
    A model that cannot give a second handle (the `small` U-Net, several gpu_ids, stand-ins) gets one lane on the current stream: enqueue, wait, hand out.

    ``jpeg_quality`` (1..100, Pillow's default is 75; or a ``jpeg.JpegOptions`` with Pillow's ``optimize`` / restart switches and ``subsampling``, which also lifts the multiples-of-16 rule: any ``out_size`` then encodes): every lane encodes its frames on its own stream right behind the generator (jpeg.JpegEncoder,
    include/lspjpeg.h) and the frames are handed out as complete JPEG files (``bytes``, what demo.py:271's save_images writes as pred_<n>.jpg); only the
    compressed bytes cross PCIe.  There is no host encoder: a model on the host with ``jpeg_quality`` raises.

    ``video`` (a video.AviWriter; demo.py:275-285): the encoded frames go into that Motion-JPEG AVI instead of being handed out -- each lane muxes its batch
    on the device behind the encoder (video.DeviceMuxer, include/lspavi.h) and the fragments are appended in frame order; ``jpeg_quality`` defaults to 75,
    the function returns [] (``on_frame(i, None)`` is still called per frame).  ``audio``: the CLIP's float32 waveform at the writer's rate (tensor or
    array), required exactly when the writer has an audio stream; frame k of the file carries its samples [k * rate // fps, (k + 1) * rate // fps).
    ``video_route`` "device" / "host" (JpegEncoder.collect + AviWriter.append_jpegs) overrides video.DEFAULT_VIDEO_ROUTE; both write the same file.

    ``out_size`` (an int or ``(width, height)``, as Pillow's ``size``; None: off) with ``resample`` ("box", "bilinear", "hamming", "bicubic", "lanczos"): every lane
    resamples its batch on its own stream right behind the generator (resize.Resizer, include/lspresize.h: ``Image.resize``, bit for bit) into a buffer it owns; the host
    copy, the JPEG encoder and the video sink then see ``out_size`` frames, and ``video`` must be a writer of that geometry.

    ``png`` (True or a ``png.PngOptions``; None: off): as ``jpeg_quality``, but the frames leave as PNG files, losslessly (png.PngEncoder, include/lsppngenc.h): Pillow
    reads back exactly the frames the call returns without it.  Frames of any ``out_size``.  Not together with ``jpeg_quality`` or ``video``, and not on a host model."""
    device = device or cand_image.device
    frames: List[np.ndarray] = []
    idx = 0
    on_gpu = device.type == "cuda"
    png = _check_png(png, jpeg_quality, video, on_gpu)
    if out_size is not None:
        out_size = _check_out_size(out_size, resample, on_gpu, video)
    if video is not None and jpeg_quality is None:
        jpeg_quality = 75
    if jpeg_quality is not None and not on_gpu:
        raise ValueError("jpeg_quality: the JPEG encoder runs on the device only, and this model renders on the host")
    if video is not None:
        from .video import VideoSink, clip_audio
        audio_dev, audio_host = clip_audio(video, audio, device)
        frame_base = video.nframes
    elif audio is not None:
        raise ValueError("audio is the sound track of ``video``: pass an AviWriter")
    nlane = max(1, int(streams)) if on_gpu and getattr(model, "supports_replicas", lambda: False)() else 1
    try:
        takes_out = "out" in inspect.signature(model.inference_image).parameters      # (stand-in models of the tests do not)
    except (TypeError, ValueError):
        takes_out = False
    lanes: List[dict] = []              # made at the first batch (shapes come from the data)

    def emit(i0, items):
        for k, item in enumerate(items):
            if on_frame is not None:
                on_frame(i0 + k, item)
            else:
                frames.append(item)

    def drain(lane):
        if lane["busy"] is not None:
            i0, n = lane["busy"]
            if lane["sink"] is not None:
                lane["sink"].collect()                          # waits for the lane's stream; one copy, appended to the file
                if on_frame is not None:
                    emit(i0, [None] * n)
            elif lane["jpeg"] is not None:
                emit(i0, lane["jpeg"].collect())                # waits for the lane's stream, then copies the compressed bytes only
            else:
                (lane["stream"] if lane["stream"] is not None else torch.cuda.current_stream(device)).synchronize()
                emit(i0, [lane["host"][k].numpy().copy() for k in range(n)])
            lane["busy"] = None

    for n, chunk in enumerate(batched(feature_maps, batch)):
        chunk = [m if m.dim() == 3 else m.unsqueeze(0) for m in chunk]
        b = len(chunk)
        if not on_gpu:                                          # (stand-in models on the host: tests)
            host = model.inference_image(torch.stack(chunk).to(device, torch.float32), cand_image)
            emit(idx, [host[k].numpy().copy() for k in range(b)])
            idx += b
            continue
        if not lanes:
            shape = (batch,) + tuple(chunk[0].shape)
            cur = torch.cuda.current_stream(device)
            for k in range(nlane):
                st = torch.cuda.Stream(device) if nlane > 1 else None
                if st is not None:
                    st.wait_stream(cur)                          # cand_image was produced there
                lanes.append({"stream": st, "busy": None, "host": None, "u8": None, "jpeg": None, "sink": None, "resizer": None, "small": None,
                              "stage": torch.empty(shape, dtype=torch.float32, pin_memory=True), "dev": torch.empty(shape, dtype=torch.float32, device=device)})
                lanes[-1]["stage_np"] = lanes[-1]["stage"].numpy()
        lane = lanes[n % nlane]
        drain(lane)                                             # its previous batch: frames handed out, buffers free
        cpu_rows = [k for k, m in enumerate(chunk) if m.device.type != "cuda"]
        for k in cpu_rows:
            # host memcpy into pinned memory (the other lanes keep rendering).  Through numpy, i.e. on THIS thread: torch's CPU copy_ fans a 1-MiB tensor out over its
            # intra-op pool (128 threads on the GPU boxes, under a 16-CPU container quota), whose spinning workers get the whole process throttled for milliseconds at a time
            # -- measured as 4-6 ms per MiB "copied" and 8-13 ms waits for a 1.5-ms forward (tools/render_loop_profile.py, tools/host_probe.py)
            m = chunk[k]
            if m.dtype == torch.float32 and m.is_contiguous():
                np.copyto(lane["stage_np"][k], m.numpy())
            else:
                lane["stage"][k].copy_(m)
        if lane["stream"] is not None and len(cpu_rows) < b:
            lane["stream"].wait_stream(torch.cuda.current_stream(device))      # maps that live on the device were produced there
        with (torch.cuda.stream(lane["stream"]) if lane["stream"] is not None else _null()):
            if len(cpu_rows) == b:
                lane["dev"][:b].copy_(lane["stage"][:b], non_blocking=True)
            else:
                for k, m in enumerate(chunk):
                    lane["dev"][k].copy_(lane["stage"][k] if m.device.type != "cuda" else m, non_blocking=True)
                    if m.device.type == "cuda" and lane["stream"] is not None:
                        m.record_stream(lane["stream"])           # read on the lane's stream: the caching allocator must not hand its memory out again before that copy ran
            kw = {"replica": n % nlane} if nlane > 1 else {}
            if takes_out:
                if lane["u8"] is None:
                    H = chunk[0].shape[-1]
                    lane["u8"] = torch.empty((batch, H, H, 3), dtype=torch.uint8, device=device)
                kw["out"] = lane["u8"][:b]
            u8 = model.inference_image(lane["dev"][:b], cand_image, **kw)
            if out_size is not None:
                if lane["resizer"] is None:
                    lane["resizer"], lane["small"] = _lane_resizer(device, batch, out_size)
                u8 = lane["resizer"].resize(u8, out_size, resample, out=lane["small"][:b])       # on the lane's stream, behind the generator
            if video is not None:
                if lane["sink"] is None:
                    lane["sink"] = VideoSink(video, tuple(u8.shape[1:3]), jpeg_quality, device, batch, audio_dev, audio_host, video_route)
                lane["sink"].submit(u8, frame_base + idx)       # on the lane's stream, behind the generator
            elif jpeg_quality is not None or png is not None:
                if lane["jpeg"] is None:
                    lane["jpeg"] = _frame_encoder(tuple(u8.shape[1:3]), 3, jpeg_quality, png, device, batch)
                lane["jpeg"].submit(u8)                         # on the lane's stream, behind the generator
            else:
                if lane["host"] is None:
                    lane["host"] = torch.empty((batch,) + tuple(u8.shape[1:]), dtype=torch.uint8, pin_memory=True)
                lane["host"][:b].copy_(u8, non_blocking=True)
        lane["busy"] = (idx, b)
        idx += b
        if nlane == 1:
            drain(lane)                                         # one lane: nothing to overlap with -- wait now (prompt) rather than behind the next batch's enqueue
    # hand out what is still in flight, oldest first
    for lane in sorted((l for l in lanes if l["busy"] is not None), key=lambda l: l["busy"][0]):
        drain(lane)
    return frames


def _check_out_size(out_size, resample, on_gpu, video):
    """(width, height) of ``out_size``; everything the resampler or the writer would refuse is refused here, before anything runs"""
    from .resize import check_filter, check_size
    check_filter(resample)
    out_size = check_size(out_size)
    if not on_gpu:
        raise ValueError("out_size: the resampler runs on the device only, and this model renders on the host")
    if video is not None and (video.width, video.height) != out_size:
        raise ValueError("video is an AviWriter of %dx%d, out_size is %dx%d" % (video.width, video.height, out_size[0], out_size[1]))
    return out_size


def _check_png(png, jpeg_quality, video, on_gpu):
    """``png=`` as a PngOptions, or None; what cannot go with it is refused here, before anything runs"""
    if png is None or png is False:
        return None
    from .png import PngOptions
    png = PngOptions.of(png)
    if jpeg_quality is not None:
        raise ValueError("png and jpeg_quality: a frame leaves as one file, PNG or JPEG")
    if video is not None:
        raise ValueError("png and video: the AVI files are Motion-JPEG")
    if not on_gpu:
        raise ValueError("png: the PNG encoder runs on the device only, and this model renders on the host")
    return png


def _frame_encoder(size, channels, jpeg_quality, png, device, batch):
    """the JPEG or the PNG encoder of one lane: the same submit / collect"""
    if png is not None:
        from .png import PngEncoder
        return PngEncoder(size, channels, device, max_batch=batch, level=png)
    from .jpeg import JpegEncoder
    return JpegEncoder(size, channels, jpeg_quality, device, max_batch=batch)


def _lane_resizer(device, batch, out_size):
    """a Resizer (its plans and workspace) and the uint8 buffer of the resized frames, both owned by one lane"""
    from .resize import Resizer
    return Resizer(device, max_batch=batch), torch.empty((batch, out_size[1], out_size[0], 3), dtype=torch.uint8, device=device)


class _null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


def render_frames_from_landmarks(model, landmarks: Iterable, shoulders: Iterable, cand_image: torch.Tensor,
                                 pad=None, load_size: int = 512, batch: int = 8,
                                 on_frame: Optional[Callable[[int, np.ndarray], None]] = None,
                                 jpeg_quality=None, save_input: bool = False, video=None, audio=None, video_input=None,
                                 video_route: Optional[str] = None, out_size=None, resample: str = "bicubic", png=None) -> List[np.ndarray]:
    """demo.py:260-272 with the edge map drawn on the device: per frame the loop moves the 73 landmarks and the shoulder
    points (~1.5 KB) instead of a host-rasterised 1 MiB feature map.  ``landmarks`` yields [73, 2] arrays (``pred_landmarks[i]``
    of demo.py:262), ``shoulders`` yields [n, 2] arrays (``pred_shoulders[i]``); ``pad`` as ``facedataset.dataset.image_pad``.

    ``jpeg_quality``: frames are encoded on the device behind the generator and handed out as JPEG files (``bytes``, see render_frames).
    ``save_input`` (``Image2Image.save_input``, demo.py:269-270): every frame is a ``(pred, input)`` pair, ``input`` the uint8 edge map
    ``np.uint8(map * 255)`` -- written by the rasteriser in the same launch as the float map, and JPEG-encoded (grayscale) with ``jpeg_quality``.

    ``video`` / ``audio`` / ``video_route`` as render_frames: the frames go into that AviWriter (``jpeg_quality`` defaults to 75) and the function returns [];
    with ``save_input`` a second, grayscale writer for the edge maps may be passed as ``video_input`` (it gets the same ``audio`` if it has an audio stream).

    ``out_size`` / ``resample`` as render_frames: the frames are resampled behind the generator and leave (host copy, JPEG, ``video``) at ``out_size``; the edge maps
    of ``save_input`` / ``video_input`` stay ``load_size``.

    ``png`` as render_frames: the frames are handed out as PNG files, and with ``save_input`` the edge maps as grey PNG files, both lossless."""
    from .feature_map import FeatureMapRasteriser
    device = cand_image.device
    png = _check_png(png, jpeg_quality, video, device.type == "cuda")
    if out_size is not None:
        out_size = _check_out_size(out_size, resample, device.type == "cuda", video)
    resizer = small = None
    if video is not None and jpeg_quality is None:
        jpeg_quality = 75
    if video_input is not None and not (save_input and video is not None):
        raise ValueError("video_input is the edge maps' file: it needs save_input=True and video")
    if video is None and audio is not None:
        raise ValueError("audio is the sound track of ``video``: pass an AviWriter")
    if jpeg_quality is not None and device.type != "cuda":
        raise ValueError("jpeg_quality: the JPEG encoder runs on the device only")
    rast = None
    maps_buf = edge_buf = None
    enc = enc_in = None
    sink = sink_in = None
    if video is not None:
        from .video import VideoSink, clip_audio
        tracks = clip_audio(video, audio, device)
        tracks_in = clip_audio(video_input, audio if video_input.has_audio else None, device) if video_input is not None else None
        bases = (video.nframes, video_input.nframes if video_input is not None else 0)

    def chunks():
        nonlocal rast, maps_buf, edge_buf
        for lm, sh in zip(batched(landmarks, batch), batched(shoulders, batch)):
            lm_a, sh_a = np.stack([np.asarray(x) for x in lm]), np.stack([np.asarray(x) for x in sh])
            b = lm_a.shape[0]
            if rast is None:
                rast = FeatureMapRasteriser(load_size, sh_a.shape[1], device)
                maps_buf = torch.empty((batch, 1, load_size, load_size), dtype=torch.float32, device=device)
                if save_input:
                    edge_buf = torch.empty((batch, load_size, load_size), dtype=torch.uint8, device=device)
            edges = edge_buf[:b] if save_input else None
            yield rast.rasterise(lm_a, sh_a, pad, out=maps_buf[:b], out_u8=edges), edges

    frames: List[np.ndarray] = []
    idx = 0
    host = host_in = None                                       # pinned result tensors, reused
    for maps, edges in chunks():
        u8 = model.inference_image(maps, cand_image)
        b = u8.shape[0]
        if out_size is not None:
            if resizer is None:
                resizer, small = _lane_resizer(device, batch, out_size)
            u8 = resizer.resize(u8, out_size, resample, out=small[:b])
        if video is not None:
            if sink is None:
                sink = VideoSink(video, tuple(u8.shape[1:3]), jpeg_quality, device, batch, tracks[0], tracks[1], video_route)
                if video_input is not None:
                    sink_in = VideoSink(video_input, load_size, jpeg_quality, device, batch, tracks_in[0], tracks_in[1], video_route)
            sink.submit(u8, bases[0] + idx)
            if sink_in is not None:
                sink_in.submit(edges, bases[1] + idx)
            # one batch at a time: the rasteriser's output tensors are reused, and collect() waits on the stream's own tail
            sink.collect()
            if sink_in is not None:
                sink_in.collect()
            if on_frame is not None:
                for k in range(b):
                    on_frame(idx + k, None)
            idx += b
            continue
        if jpeg_quality is not None or png is not None:
            if enc is None:
                enc = _frame_encoder(tuple(u8.shape[1:3]), 3, jpeg_quality, png, device, batch)
                enc_in = _frame_encoder(load_size, 1, jpeg_quality, png, device, batch) if save_input else None
            enc.submit(u8)
            if save_input:
                enc_in.submit(edges)
            # one batch at a time: the rasteriser's output tensors are reused, and collect() waits on the stream's own tail
            preds = enc.collect()
            items = list(zip(preds, enc_in.collect())) if save_input else preds
        else:
            if host is None:
                host = torch.empty((batch,) + tuple(u8.shape[1:]), dtype=torch.uint8, pin_memory=True)
                host_in = torch.empty((batch, load_size, load_size), dtype=torch.uint8, pin_memory=True) if save_input else None
            host[:b].copy_(u8, non_blocking=True)
            if save_input:
                host_in[:b].copy_(edges, non_blocking=True)
            # one batch at a time: the rasteriser's output tensor is reused, and the wait is on the stream's own tail
            torch.cuda.current_stream(device).synchronize()
            items = [host[k].numpy().copy() for k in range(b)]
            if save_input:
                items = [(items[k], host_in[k].numpy().copy()) for k in range(b)]
        for k, item in enumerate(items):
            (on_frame(idx + k, item) if on_frame else frames.append(item))
        idx += b
    return frames
