"""lspavi_pack_multi (include/lspavi.h, livespeechportraits_amd/video.py DeviceMultiMuxer): one encoded batch, split into runs, becomes one
fragment per run, the audio taken from per-run rings.  Every fragment and its index must equal, byte for byte, (a) what AviWriter builds on
the host from the linearised waveform (pinned on the strict parser and on Pillow by tests/test_avi_cpu.py) and (b) what lspavi_pack gives for
that run alone.  The whole output buffer is compared, so the bytes between and above the fragments are covered.  Nothing has a tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import jpeg_model as M
from test_avi_cpu import GEOMETRIES, SPECIAL
from test_gpu_avi import host_fragment

pytestmark = pytest.mark.gpu

RATE, FPS = 16000, 60
s = lambda f: f * RATE // FPS


@functools.lru_cache(None)
def material(geom):
    """64 frames whose JPEG lengths alternate in parity (so every run of two or more holds both), and their files"""
    h, w, ch = GEOMETRIES[geom]
    pix = [np.random.default_rng(seed).integers(0, 256, (h, w, 3) if ch == 3 else (h, w), dtype=np.uint8) for seed in range(110)]
    files = [M.encode(p, 75) for p in pix]
    odd, even = [k for k, f in enumerate(files) if len(f) & 1], [k for k, f in enumerate(files) if not len(f) & 1]
    assert len(odd) >= 32 and len(even) >= 32, (len(odd), len(even))
    order = [k for pair in zip(odd[:32], even[:32]) for k in pair]
    return np.stack([pix[k] for k in order]), [files[k] for k in order]


def stream_of(n, seed):
    x = (np.random.default_rng(seed).standard_normal(n) * 0.4).astype(np.float32)
    for at in range(seed % 7, n - SPECIAL.size, 131):           # NaN, +-1.5, +-1.0, infinities and rounding ties in every chunk
        x[at:at + SPECIAL.size] = SPECIAL
    return x


class Run:
    """one run of a case: ``count`` frames from the file's ``frame0``, ``fmt``, the stream sample of the file's frame 0, and how many
    samples the ring holds beyond the run's span"""

    def __init__(self, count, frame0=0, fmt="f32", sample0=0, slack=5):
        self.count, self.frame0, self.fmt, self.sample0, self.slack = count, frame0, fmt, sample0, slack
        self.first, self.last = sample0 + s(frame0), sample0 + s(frame0 + count)

    def ring(self, j, ring_samples, device):
        """(device ring, avail_begin, avail_end, the FILE's linear waveform).  Ring positions outside [begin, end) hold 7.0."""
        stream = stream_of(self.last + self.slack + 8, 11 + j)
        end = self.last + self.slack
        begin = max(0, end - ring_samples)
        assert begin <= self.first, "the case does not fit its ring"
        ring = np.full(ring_samples, 7.0, np.float32)
        idx = np.arange(begin, end)
        ring[idx % ring_samples] = stream[idx]
        return torch.from_numpy(ring).to(device), begin, end, stream[self.sample0:]


def wrap_offset(run, ring_samples):
    """samples between the run's first sample and the ring's wrap point inside its span (None: the span does not wrap)"""
    d = -run.first % ring_samples
    return d if d < run.last - run.first else None


def check(gpu_device, tmp_path, geom, runs, ring_samples):
    from livespeechportraits_amd.jpeg import JpegEncoder
    from livespeechportraits_amd.video import DeviceMultiMuxer, DeviceMuxer
    h, w, ch = GEOMETRIES[geom]
    pixels, files = material(geom)
    batch = sum(r.count for r in runs)
    frames_dev = torch.from_numpy(pixels[:batch]).to(gpu_device)
    enc = JpegEncoder((h, w), ch, 75, gpu_device, max_batch=batch)
    mux = DeviceMultiMuxer(enc)
    table, want, at = [], [], 0
    for j, r in enumerate(runs):
        part = files[at:at + r.count]
        if r.count >= 2:
            assert {len(f) & 1 for f in part} == {0, 1}
        ring, begin, end, wave = (None, 0, 0, None) if r.fmt is None else r.ring(j, ring_samples, gpu_device)
        table.append((r.count, r.frame0, r.fmt, ring, r.sample0, begin, end))
        host = host_fragment(tmp_path, geom, part, r.fmt, wave, r.frame0)
        # the same run alone through lspavi_pack, from the linearised waveform
        one = JpegEncoder((h, w), ch, 75, gpu_device, max_batch=r.count)
        single = DeviceMuxer(one, r.fmt)
        single.submit(frames_dev[at:at + r.count], r.frame0, None if r.fmt is None else torch.from_numpy(np.ascontiguousarray(wave)).to(gpu_device))
        data, index, *rest = single.collect()
        assert (data.tobytes(), index.tobytes(), tuple(rest)) == (host[0], host[1].tobytes(), tuple(host[2:])), ("lspavi_pack", j)
        one.close()
        want.append(host)
        at += r.count
    expect = np.full(mux.capacity, 0xA5, np.uint8)
    offs, pos = [], 0
    for frag in want:
        offs.append(pos)
        expect[pos:pos + len(frag[0])] = np.frombuffer(frag[0], np.uint8)
        pos = (pos + len(frag[0]) + 15) & ~15
    assert mux.capacity - pos >= 16
    mux._out.fill_(0xA5)
    got = []
    for _ in range(2):                                          # twice into the same buffer, not refilled
        out = mux.pack(frames_dev, table)
        got.append([(d.tobytes(), i.tobytes(), tuple(int(v) for v in rest)) for d, i, *rest in out])
        buf = mux._out.cpu().numpy()
        bad = np.flatnonzero(buf != expect)
        assert bad.size == 0, "first differing byte of the buffer at %d (fragments start at %s)" % (bad[0], offs)
    assert got[0] == got[1]
    for j, frag in enumerate(want):
        assert got[0][j] == (frag[0], frag[1].tobytes(), tuple(int(v) for v in frag[2:])), j
    enc.close()


F, S, N = "f32", "s16", None
LAYOUTS = {
    "one": [Run(5, 0, F, 3)],
    "two": [Run(1, 7, S, 1), Run(2, 0, N)],
    "three": [Run(2, 7, F, 2), Run(5, 0, S, 0), Run(1, 7, N)],
    "sixteen": [Run(1, (0, 7)[j & 1], (F, S, N)[j % 3], 100 * j + j % 4) for j in range(16)],
    "batch64": [Run(n, (0, 7, 3)[j % 3], (S, F, N, F)[j % 4], 1000 * j + (j + 1) % 4) for j, n in enumerate([1, 2, 5, 1, 2, 5, 1, 2, 5, 1, 2, 5, 8, 8, 8, 8])],
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("geom", ["c16", "g8"])
def test_fragments_equal_the_host_and_the_single_file_muxer(gpu_device, tmp_path, geom, layout):
    runs = LAYOUTS[layout]
    assert layout != "batch64" or sum(r.count for r in runs) == 64
    check(gpu_device, tmp_path, geom, runs, ring_samples=4096)


def _sample0_for(frame0, d):
    """The smallest sample0 >= 600 with (sample0 + s(frame0) + d) % 600 == 0: a ring of 600 samples then wraps ``d`` samples into a run
    that starts at the file's ``frame0``.  Runs of two frames (533 or 534 samples) fit that ring.  d = 0 and d = the first frame's sample
    count put the wrap exactly on a chunk boundary; the others put it inside the first or the second frame's chunk.  Chunk starts are even
    and a sample takes 2 or 4 bytes, so the wrap's byte phase inside a 16-byte piece is even: 8 phases."""
    return 600 + (-(600 + s(frame0) + d)) % 600


WRAPS = [(fmt, frame0, d) for fmt in (S, F) for frame0 in (0, 7)
         for d in (0, s(frame0 + 1) - s(frame0)) + tuple(range(1, 9)) + tuple(range(s(frame0 + 1) - s(frame0) + 1, s(frame0 + 1) - s(frame0) + 9))]


def test_the_wrap_cases_cover_every_phase_and_both_boundaries(tmp_path):
    """no device: where the wrap falls in the OUTPUT, from the host fragment's own index"""
    for geom in ("c16", "g8"):
        _, files = material(geom)
        phases = {S: set(), F: set()}
        boundary = set()
        residues = set()
        for fmt, frame0, d in WRAPS:
            run = Run(2, frame0, fmt, _sample0_for(frame0, d), slack=40)
            assert wrap_offset(run, 600) == d
            residues.add(run.sample0 % 4)
            n0 = s(frame0 + 1) - s(frame0)
            frag = host_fragment(tmp_path, geom, files[:2], fmt, stream_of(run.last + 8, 1)[run.sample0:], frame0)
            audio = [int(o) for ck, _, o, _ in frag[1] if ck == 0x62773130]
            bps = 4 if fmt == F else 2
            if d in (0, n0):
                boundary.add((fmt, d == 0))
                continue
            at = audio[0] + 8 + d * bps if d < n0 else audio[1] + 8 + (d - n0) * bps
            phases[fmt].add(at % 16)
        assert phases[S] == set(range(0, 16, 2)), (geom, phases)
        assert phases[F] >= {0, 4, 8, 12} and len(phases[F]) >= 4, (geom, phases)
        assert boundary == {(S, True), (S, False), (F, True), (F, False)}
        assert residues == {0, 1, 2, 3}


@pytest.mark.parametrize("fmt,frame0,d", WRAPS)
def test_the_ring_wraps_inside_a_run(gpu_device, tmp_path, fmt, frame0, d):
    run = Run(2, frame0, fmt, _sample0_for(frame0, d), slack=40)
    assert wrap_offset(run, 600) == d
    other = Run(1, 7 - frame0, S if fmt == F else F, _sample0_for(7 - frame0, 100) + 1, slack=300)     # a second file whose chunk wraps too
    assert wrap_offset(other, 600) is not None
    for geom in ("c16", "g8"):
        check(gpu_device, tmp_path, geom, [run, other], ring_samples=600)


def test_refusals_launch_nothing(gpu_device):
    from livespeechportraits_amd import _native as N
    from livespeechportraits_amd.jpeg import JpegEncoder
    from livespeechportraits_amd.video import DeviceMultiMuxer
    pixels, _ = material("c16")
    frames_dev = torch.from_numpy(pixels[:4]).to(gpu_device)
    enc = JpegEncoder(16, 3, 75, gpu_device, max_batch=32)
    mux = DeviceMultiMuxer(enc)
    ring = torch.zeros(600, dtype=torch.float32, device=gpu_device)
    for t in (mux._out, mux._ws):
        t.fill_(0xA5)
    mux._meta.fill_(-1515870811)                                # 0xA5A5A5A5
    before = [t.cpu().numpy().copy() for t in (mux._out, mux._ws, mux._meta)]
    c = ctypes.c_void_p

    def raw(batch, rows):
        """rows: (first, count, fmt, frame0, sample0, begin, end); straight into the library"""
        table = (N.AviRun * 17)()
        for t, (first, count, fmt, frame0, sample0, begin, end) in zip(table, rows):
            t.first, t.count, t.audio_format, t.frame0, t.ring_dev, t.ring_samples = first, count, fmt, frame0, ring.data_ptr() if fmt else None, 600
            t.sample0, t.avail_begin, t.avail_end = sample0, begin, end
        dst, sizes = enc.slab
        R = mux._srows
        stream = torch.cuda.current_stream(gpu_device)
        rc = mux.lib.lspavi_pack_multi(c(mux._header.data_ptr()), len(enc.header), c(dst.data_ptr()), enc.capacity, c(sizes.data_ptr()), batch,
                                       ctypes.cast(table, ctypes.POINTER(N.AviRun)), len(rows), RATE, FPS, c(mux._out.data_ptr()), mux.capacity,
                                       c(mux._meta[R:].data_ptr()), c(mux._meta.data_ptr()), c(mux._ws.data_ptr()), mux._ws_bytes, c(stream.cuda_stream))
        return rc, mux.lib.lspavi_last_error().decode()

    enc.enqueue(frames_dev)
    span = s(9) - s(7)                                          # frames 7, 8 from sample0 = 1000: samples 1000 + [s(7), s(9))
    a = 1000 + s(7)
    cases = {
        "before avail_begin": (2, [(0, 2, 3, 7, 1000, a + 1, a + 1 + 599)], "need samples"),
        "past avail_end": (2, [(0, 2, 1, 7, 1000, a - 10, a + span - 1)], "need samples"),
        "longer than the ring": (3, [(0, 3, 3, 7, 1000, a, a + 600)], "need samples"),
        "more than the ring holds": (2, [(0, 2, 3, 7, 1000, a, a + 601)], "cannot hold"),
        "runs leave a gap": (4, [(0, 1, 0, 0, 0, 0, 0), (2, 2, 0, 0, 0, 0, 0)], "cover the batch"),
        "runs stop short": (4, [(0, 1, 0, 0, 0, 0, 0), (1, 2, 0, 0, 0, 0, 0)], "cover 3 frames"),
        "runs pass the batch": (4, [(0, 1, 0, 0, 0, 0, 0), (1, 4, 0, 0, 0, 0, 0)], "cover the batch"),
        "17 runs": (17, [(j, 1, 0, 0, 0, 0, 0) for j in range(17)], "1..16 runs"),
        "count 0": (4, [(0, 4, 0, 0, 0, 0, 0), (4, 0, 0, 0, 0, 0, 0)], "count"),
        "an unknown format": (1, [(0, 1, 2, 0, 0, 0, 0)], "audio_format"),
    }
    for name, (batch, rows, words) in cases.items():
        rc, msg = raw(batch, rows)
        assert rc == -1 and words in msg, (name, rc, msg)
    torch.cuda.synchronize()
    after = [t.cpu().numpy() for t in (mux._out, mux._ws, mux._meta)]
    assert all(np.array_equal(x, y) for x, y in zip(before, after)), "a refused call wrote to a device buffer"
    with pytest.raises(N.LspaviError, match="need samples"):
        mux.pack(frames_dev[:2], [(2, 7, "f32", ring, 1000, a + 1, a + 600)])
    with pytest.raises(ValueError, match="runs"):
        mux.pack(frames_dev[:2], [])
    assert raw(2, [(0, 2, 3, 7, 1000, a, a + span)])[0] == 0     # exactly enough: accepted
    torch.cuda.synchronize()
    assert int(mux._meta.cpu().numpy().view(np.uint32)[0, 2]) == 4
    assert mux.lib.lspavi_capacity_bytes_multi(len(enc.header), enc.capacity, 4, 5, RATE, FPS) == 0
    assert mux.lib.lspavi_capacity_bytes_multi(len(enc.header), enc.capacity, 4, 4, RATE, FPS) == \
        mux.lib.lspavi_capacity_bytes(len(enc.header), enc.capacity, 4, 3, RATE, FPS) + 80
    enc.close()
