"""The candidate images of demo.py:88-95 on the device::

    for j in range(4):
        output = imread(os.path.join(data_root, 'candidates', f'normalized_full_{j}.jpg'))
        output = albumentations.pytorch.transforms.ToTensor(normalize={'mean': (0.5, 0.5, 0.5), 'std': (0.5, 0.5, 0.5)})(image=output)['image']
        img_candidates.append(output)
    img_candidates = torch.cat(img_candidates).unsqueeze(0)          # [1, 12, 512, 512]

``load_candidates`` decodes the four files with jpeg.JpegDecoder (the pixels Pillow returns, bit for bit) straight into channels
3j .. 3j + 2 of the float tensor, through a 256-entry table that holds the normalisation: no uint8 image and no host tensor in
between.  The table is ``float32(float64(v) / 255.0)``, then ``(t - 0.5f) / 0.5f`` in float32 -- what ToTensor(normalize=...)
computes (``img / 255.0`` then ``F.normalize``).  albumentations is not installed where this is built, so the table is
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


def load_candidates(paths_or_data_root: Union[str, Sequence], device="cuda:0", size: int = 512, decoder=None) -> torch.Tensor:
    """float32 ``[1, 12, size, size]`` on ``device`` from four JPEG files: a data root (``<root>/candidates/normalized_full_{0..3}.jpg``), four
    paths, or four ``bytes`` objects.  Files that are not 3-component ``size`` x ``size`` are refused (ValueError); files the decoder
    cannot take raise jpeg.JpegError."""
    from .jpeg import JpegDecoder, probe
    src = candidate_paths(paths_or_data_root) if isinstance(paths_or_data_root, (str, os.PathLike)) else list(paths_or_data_root)
    if len(src) != CANDIDATES:
        raise ValueError("%d candidate images, demo.py reads %d" % (len(src), CANDIDATES))
    files = []
    for s in src:
        if isinstance(s, (bytes, bytearray, memoryview)):
            files.append(bytes(s))
        else:
            with open(s, "rb") as f:
                files.append(f.read())
    for j, data in enumerate(files):
        i = probe(data)
        if i.status == 0 and (i.width, i.height, i.components) != (size, size, 3):
            raise ValueError("candidate %d is %dx%d with %d components, the generator takes %dx%d RGB" % (j, i.width, i.height, i.components, size, size))
    device = torch.device(device)
    decoder = decoder or JpegDecoder(device, max_side=size, max_batch=CANDIDATES)
    out = torch.empty((3 * CANDIDATES, size, size), dtype=torch.float32, device=device)
    table = torch.from_numpy(normalisation_table()).to(device)
    decoder.decode_into(files, out, 0, table)
    return out.unsqueeze(0)
