"""The candidate images of demo.py:88-95 on the device (``png=True``: PNG files as well, through png.PngDecoder)::

    for j in range(4):
        output = imread(os.path.join(data_root, 'candidates', f'normalized_full_{j}.jpg'))
        output = albumentations.pytorch.transforms.ToTensor(normalize={'mean': (0.5, 0.5, 0.5), 'std': (0.5, 0.5, 0.5)})(image=output)['image']
        img_candidates.append(output)
    img_candidates = torch.cat(img_candidates).unsqueeze(0)          # [1, 12, 512, 512]

``load_candidates`` decodes the four files with jpeg.JpegDecoder (the pixels Pillow returns, bit for bit) straight into channels
3j .. 3j + 2 of the float tensor, through a 256-entry table that holds the normalisation: no uint8 image and no host tensor in
between.  The table is ``float32(float64(v) / 255.0)``, then ``(t - 0.5f) / 0.5f`` in float32 -- what ToTensor(normalize=...)
computes (``img / 255.0`` then ``F.normalize``).  With ``resize=`` a photograph of any size the decoder takes is decoded at its own size
and resampled on the device to ``size`` x ``size`` (resize.Resizer: ``Image.open(f).resize((size, size), filter)``, bit for bit), its pixels
going through the same table into the same channels.  albumentations is not installed where this is built, so the table is
*parity-unpinned against albumentations*: it is pinned on that formula (tests/test_jpeg_decode_cpu.py).
"""
from __future__ import annotations

import os
from typing import Sequence, Union

import numpy as np
import torch

CANDIDATES = 4


def normalisation_table() -> np.ndarray:
    """float32 [256]: pixel value -> ToTensor(normalize mean 0.5, std 0.5)"""
    t = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    return (t - np.float32(0.5)) / np.float32(0.5)


def candidate_paths(data_root: str) -> list:
    return [os.path.join(data_root, "candidates", "normalized_full_%d.jpg" % j) for j in range(CANDIDATES)]


def load_candidates(paths_or_data_root: Union[str, Sequence], device="cuda:0", size: int = 512, decoder=None, resize=None, resizer=None,
                    progressive: bool = False, parallel: bool = False, png: bool = False, png_decoder=None) -> torch.Tensor:
    """float32 ``[1, 12, size, size]`` on ``device`` from four JPEG files: a data root (``<root>/candidates/normalized_full_{0..3}.jpg``), four
    paths, or four ``bytes`` objects.  Files that are not 3-component ``size`` x ``size`` are refused (ValueError); files the decoder
    cannot take raise jpeg.JpegError.

    ``resize`` ("box", "bilinear", "hamming", "bicubic" or "lanczos"; None: off): the files may have any geometry the decoder takes, each its
    own; a file that is not ``size`` x ``size`` is resampled to it as ``Image.resize((size, size), filter)`` does, one that is takes the path
    above.  ``resizer``: a resize.Resizer to reuse.

    ``progressive``: complete progressive files (SOF2, what photo tools and the web mostly export) are taken as well, to the pixels Pillow
    returns for them; handed on to the decoder this call creates (a ``decoder`` passed in decides for itself).

    ``parallel``: the decoder this call creates decodes inside each file in parallel (jpeg.JpegDecoder's ``parallel``); the tensor is the same.

    ``png`` (off by default; without it nothing changes): a file that starts with the PNG signature goes to a png.PngDecoder (``png_decoder``, or
    this call's own), every other file to the JPEG decoder as before; the two kinds mix within the four candidates.  A PNG must give 3 components
    (colour types 2, 3, 6) and be ``size`` x ``size`` unless ``resize`` is set, with which it is decoded at its own size and resampled exactly as
    a JPEG is; a PNG the decoder refuses raises png.PngError.  Given a data root, candidate j is ``normalized_full_{j}.jpg`` if that exists, else
    ``normalized_full_{j}.png``."""
    from . import jpeg as J
    P = None
    if png:
        from . import png as P
    if resize is not None:
        from .resize import Resizer, check_filter
        resize = check_filter(resize)
    if isinstance(paths_or_data_root, (str, os.PathLike)):
        src = candidate_paths(paths_or_data_root)
        if png:
            src = [path if os.path.exists(path) else path[:-4] + ".png" for path in src]
    else:
        src = list(paths_or_data_root)
    if len(src) != CANDIDATES:
        raise ValueError("%d candidate images, demo.py reads %d" % (len(src), CANDIDATES))
    files = []
    for s in src:
        if isinstance(s, (bytes, bytearray, memoryview)):
            files.append(bytes(s))
        else:
            with open(s, "rb") as f:
                files.append(f.read())
    is_png = [png and data.startswith(P.SIGNATURE) for data in files]
    other = []                                                  # the files to resample
    for j, data in enumerate(files):
        i = P.probe(data) if is_png[j] else J.probe(data, progressive if decoder is None else getattr(decoder, "progressive", False))
        if i.status == 0 and (i.width, i.height, i.components) != (size, size, 3):
            if resize is None or i.components != 3:
                raise ValueError("candidate %d is %dx%d with %d components, the generator takes %dx%d RGB" % (j, i.width, i.height, i.components, size, size))
            other.append((j, max(i.width, i.height)))
    device = torch.device(device)
    side = max([size] + [s for _, s in other])
    if not all(is_png):
        decoder = decoder or J.JpegDecoder(device, max_side=side, max_batch=CANDIDATES, progressive=progressive, parallel=parallel)
    if any(is_png):
        png_decoder = png_decoder or P.PngDecoder(device, max_side=side, max_batch=CANDIDATES)
    out = torch.empty((3 * CANDIDATES, size, size), dtype=torch.float32, device=device)
    table = torch.from_numpy(normalisation_table()).to(device)
    resample = [j for j, _ in other]
    j = 0
    while j < CANDIDATES:                                       # runs of one kind that need no resampling: one call each
        if j in resample:
            j += 1
            continue
        k = j
        while k < CANDIDATES and is_png[k] == is_png[j] and k not in resample:
            k += 1
        (png_decoder if is_png[j] else decoder).decode_into(files[j:k], out, 3 * j, table)
        j = k
    if other:
        resizer = resizer or Resizer(device, max_batch=1)
        for kind, dec in ((True, png_decoder), (False, decoder)):
            mine = [j for j in resample if is_png[j] == kind]
            if mine:
                for j, pixels in zip(mine, dec.decode([files[j] for j in mine])):
                    resizer.resize_planes(pixels, size, table, out[3 * j:3 * j + 3], resize)
    return out.unsqueeze(0)
