"""The host side of live recording (livespeechportraits_amd/video.py: RingBook, LiveRecording, live_ring_samples, AviWriter.room_for), without
a device: the audio rings' account, the ``sample0`` rule, the ring-size formula against the schedulers' own arithmetic, and rollover."""
import numpy as np
import pytest

import avi_parser as P
from test_avi_cpu import make_files

from livespeechportraits_amd.landmarks import LandmarkScheduler
from livespeechportraits_amd.live_pool import PoolPlanner
from livespeechportraits_amd.video import AviFull, AviWriter, LiveRecording, RingBook, frame_sample, live_ring_samples

RATE, FPS = 16000, 60
s = lambda f: f * RATE // FPS
FF_MOUTH, FF_HEAD, RADII, MAX_PUSH = 18, 15, (10, 40, 20), 64
MAX_TICK = (MAX_PUSH - FF_MOUTH - 2) * RATE // FPS                     # LivePortraitPool.max_tick_samples


def test_ring_bookkeeping():
    book = RingBook(600)
    assert book.avail == (0, 0) and book.positions(0, 0).size == 0
    ring, stream = np.full(600, np.nan, np.float32), np.arange(5000, dtype=np.float32)
    for n in (0, 266, 267, 1, 600, 599, 333):
        first = book.pushed
        at = book.push(n)
        assert at.shape == (n,) and np.array_equal(at, np.arange(first, first + n) % 600)
        ring[at] = stream[first:first + n]
        begin, end = book.avail
        assert (begin, end) == (max(0, book.pushed - 600), book.pushed)
        assert np.array_equal(ring[book.positions(begin, end)], stream[begin:end])          # what it says it holds, it holds
    begin, end = book.avail
    assert end - begin == 600
    for a, b in ((begin - 1, end), (begin, end + 1), (end, begin)):
        with pytest.raises(ValueError, match="not in the ring"):
            book.positions(a, b)
    with pytest.raises(ValueError, match="does not fit"):
        book.push(601)
    with pytest.raises(ValueError):
        RingBook(0)


def test_sample0_is_at_most_one_sample_off_the_streams_own_numbering():
    F, k = np.meshgrid(np.arange(5000), np.arange(300), indexing="ij")
    d = (s(F) + s(k)) - s(F + k)
    assert d.min() == -1 and d.max() == 0                               # a file that starts late never reads ahead of the stream's rule
    N = np.arange(400000)
    n = (N / 16000 * 60).astype(np.int64)                               # live.py's frame count of a finished session
    assert [int(v) for v in n[::997]] == [int(v / 16000 * 60) for v in N[::997]]
    assert (s(n) <= N).all()                                            # the last frame's audio always exists: no zero-fill rule


def test_a_recording_spans_its_files_own_frames(tmp_path):
    files = make_files("c16")
    with AviWriter(str(tmp_path / "a.avi"), 16, 16) as w:
        rec = LiveRecording(3, "video", w, None, 1234)
        assert rec.base == 1234 and rec.sample0 == frame_sample(1234, RATE, FPS)
        assert rec.span(2) == (rec.sample0, rec.sample0 + s(2))
        w.append_jpegs(files[:2], np.zeros(s(2), np.float32))
        assert rec.span(3) == (rec.sample0 + s(2), rec.sample0 + s(5))
        nbytes, nchunks = rec.worst_case(3, 1000)
        assert (nbytes, nchunks) == (3 * (8 + 1000 + 1) + 3 * 8 + (s(5) - s(2)) * 4, 6)
        with pytest.raises(ValueError, match="empty file"):
            LiveRecording(3, "video", w, None, 0)
    with AviWriter(str(tmp_path / "b.avi"), 16, 16, channels=1, audio_rate=None) as w:
        rec = LiveRecording(0, "video_input", w, None, 77)
        assert rec.span(4) == (0, 0) and rec.worst_case(4, 500) == (4 * 509, 4)


def test_room_for_is_append_fragments_own_rule(tmp_path):
    files, wave = make_files("c16"), np.zeros(s(8), np.float32)
    probe = AviWriter(str(tmp_path / "p.avi"), 16, 16)
    frag = probe.build_fragment(files[:3], wave[:s(3)])
    exact = probe._riff_size(len(frag[0]), 6)                           # the file's size field with that fragment, closed
    probe.close()
    for max_bytes, fits in ((exact, True), (exact - 1, False)):
        w = AviWriter(str(tmp_path / "w.avi"), 16, 16, max_bytes=max_bytes)
        assert w.room_for(len(frag[0]), 6) is fits
        assert w.room_for(0, 0) and not w.room_for(len(frag[0]) + 2, 6) and not w.room_for(len(frag[0]), 7)
        if fits:
            w.append_fragment(*frag)
            assert not w.room_for(2, 0)
        else:
            with pytest.raises(AviFull):
                w.append_fragment(*frag)
        w.close()
        assert len(open(tmp_path / "w.avi", "rb").read()) == (exact + 8 if fits else exact + 8 - len(frag[0]) - 6 * 16)


def schedule(pushes, radii=RADII, max_lookahead=None):
    """(samples pushed so far, first emitted frame, frames emitted) per tick of one session, from the pool's own host arithmetic: the audio
    planner's row counts pushed through the landmark scheduler, as LivePortraitPool._dry_run does; the last push finishes the session"""
    plan = PoolPlanner(1, FF_MOUTH, FF_HEAD, 255, 16000, 16)
    sid = plan.open()
    lm = LandmarkScheduler(*radii, ring_rows=2 * max(radii) + 2 + MAX_PUSH + 32, max_lookahead=max_lookahead)
    pushed = 0
    for i, n in enumerate(pushes):
        fin = {sid} if i == len(pushes) - 1 else set()
        mouth, poses = plan.preview({sid: n}, fin)[sid]
        plan.rounds({sid: n}, fin)
        step = lm.push(mouth, poses, bool(fin))
        pushed += n
        yield pushed, step.emit0, step.n_emit
    assert lm.e == int(pushed / 16000 * 60) - FF_HEAD or lm.e == 0      # every frame of the clip came out (the poses end ff_head early)


def _pieces(total, top, seed):
    rng, out = np.random.default_rng(seed), []
    while total > 0:
        out.append(min(total, int(rng.integers(0, top + 1))))
        total -= out[-1]
    return out


SCHEDULES = {
    "a frame per tick": [266 + (k % 3 == 2) for k in range(700)],
    "bursts": _pieces(150000, 4000, 1),
    "large bursts": _pieces(400000, MAX_TICK, 2),
    "silence then the most a tick takes": [0, 0, 300, 0, MAX_TICK, MAX_TICK, 5, MAX_TICK, 0, 0, 1, MAX_TICK],
    "the clip at once": [MAX_TICK],
}


@pytest.mark.parametrize("max_lookahead", [None, 5])
@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_the_ring_holds_every_emitted_frames_span(name, max_lookahead):
    """ring_samples = max_tick_samples + (lag + 4) * ceil(rate / fps): when a frame is emitted its span is still in the ring, for a file
    that starts at frame 0 and for files that start at any later frame (their spans lie up to one sample earlier)"""
    lag = max(FF_MOUTH, FF_HEAD) + max(RADII)
    ring = live_ring_samples(lag, MAX_TICK, RATE, FPS)
    assert ring == MAX_TICK + (lag + 4) * 267
    slack, frames, empty = [], 0, 0
    for pushed, emit0, n in schedule(SCHEDULES[name], max_lookahead=max_lookahead):
        book = RingBook(ring)
        book.pushed = pushed
        begin, end = book.avail
        empty += n == 0
        for base in {0, emit0 // 2, emit0}:
            for k in range(emit0, emit0 + n):
                a, b = s(base) + s(k - base), s(base) + s(k - base + 1)
                assert begin <= a and b <= end, (name, pushed, k, base)
            if n and begin:
                slack.append(s(base) + s(emit0 - base) - begin)
        frames += n
    if len(SCHEDULES[name]) > 1:
        assert frames > 100 and empty > 0
    print(name, max_lookahead, "least room to spare:", min(slack) if slack else None)
    if name == "silence then the most a tick takes" and max_lookahead is None:   # full pushes back to back: the formula is not generous either
        assert min(slack) < 8 * 267, "the formula keeps far more than it needs: %d samples to spare" % min(slack)


def test_rollover_splits_the_session_into_files_whose_audio_joins_up(tmp_path):
    """a recorded session as LivePortraitPool drives it on the host route: groups of at most 4 frames, make_room before each run; the file is
    sized so that it fills once"""
    files = make_files("c16")
    frame_bytes = max(len(f) for f in files) + 9
    stream = (np.random.default_rng(8).standard_normal(60000) * 0.3).astype(np.float32)
    ring_samples = live_ring_samples(max(FF_MOUTH, FF_HEAD) + max(RADII), MAX_TICK, RATE, FPS)
    ring, book = np.zeros(ring_samples, np.float32), RingBook(ring_samples)
    start = 40                                                          # recording starts at the stream's frame 40
    made = []

    def writer(sid=None, which=None):
        made.append(AviWriter(str(tmp_path / ("%d.avi" % len(made))), 16, 16, max_bytes=200000))
        return made[-1]

    rec, asked = None, []
    pos = 0
    for pushed, emit0, n in schedule(_pieces(len(stream), 3000, 5)):
        ring[book.push(pushed - pos)] = stream[pos:pushed]
        pos = pushed
        if emit0 + n <= start:
            continue
        k = max(emit0, start)
        if rec is None:
            rec = LiveRecording(0, "video", writer(), lambda sid, which: asked.append((sid, which)) or writer(), k)
        while k < emit0 + n:
            take = min(4, emit0 + n - k)
            rec.make_room(take, frame_bytes, k)
            assert rec.base + rec.writer.nframes == k
            rec.writer.append_jpegs([files[f % len(files)] for f in range(k, k + take)], ring[book.positions(*rec.span(take))])
            k += take
    total = k - start
    assert asked == [(0, "video")] and len(made) == 2 and total > 150
    for w in made:
        w.close()
    parsed = [P.parse(open(w.path, "rb").read()) for w in made]
    n0, n1 = len(parsed[0]["video"]), len(parsed[1]["video"])
    assert n0 + n1 == total and n0 > 20 and n1 > 20
    assert parsed[0]["video"] + parsed[1]["video"] == [files[f % len(files)] for f in range(start, start + total)]
    # joined, the two audio streams are the pushed samples from the first file's sample0 on.  The second file's sample0 is s() of the stream
    # frame it starts at, which lies 0 or 1 samples past the first file's end (s(F) + s(k) against s(F + k)): that one sample is in no file.
    first, second = s(start), s(start + n0)
    gap = second - (first + s(n0))
    assert gap in (0, 1) and made[1].nsamples == s(n1)
    assert parsed[0]["audio"].tobytes() == stream[first:first + s(n0)].tobytes()
    assert parsed[1]["audio"].tobytes() == stream[second:second + s(n1)].tobytes()
    joined = np.concatenate([parsed[0]["audio"], stream[second - gap:second], parsed[1]["audio"]])
    assert joined.tobytes() == stream[first:second + s(n1)].tobytes()
    assert all(len(open(w.path, "rb").read()) <= 200000 for w in made)

    # no on_full: AviFull, and nothing is appended
    w = AviWriter(str(tmp_path / "full.avi"), 16, 16, max_bytes=3000)
    rec = LiveRecording(1, "video", w, None, 0)
    rec.make_room(1, frame_bytes, 0)
    with pytest.raises(AviFull, match="no on_full"):
        rec.make_room(4, frame_bytes, 0)
    # a fresh file that cannot take the run either
    rec = LiveRecording(1, "video", w, lambda sid, which: AviWriter(str(tmp_path / "tiny.avi"), 16, 16, max_bytes=3000), 0)
    with pytest.raises(AviFull, match="fresh"):
        rec.make_room(4, frame_bytes, 9)
    assert w.nframes == 0
