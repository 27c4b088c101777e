"""CPU tests of the live audio scheduler (livespeechportraits_amd/live.py): the finality rules, driven through run_plan with a
provenance backend whose stages are exact integer functions of what they read, so that any chunking of a clip can be compared
item by item with a single push, and every item's inputs can be checked against the samples pushed when it was emitted."""
import ctypes
import os
import re

import numpy as np
import pytest

from livespeechportraits_amd.live import LiveScheduler, final_windows, num_frames, run_plan, window_start

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FF_MOUTH, FF_HEAD = 18, 15
MASK = (1 << 61) - 1


def mix(*v):
    h = 1469598103934665603
    for x in v:
        h = ((h ^ (x & MASK)) * 1099511628211) & MASK
    return h


class ProvenanceBackend:
    """Every stage records what it read.  An item is (value, last sample read + 1, padded): the value folds in everything the item
    depends on, the recurrent stages every row before them."""

    def __init__(self, sched):
        self.sched = sched
        self.n = 0                       # samples pushed
        self.kept_from = 0
        self.mel_rows, self.apc_rows, self.lle_rows, self.pair_rows = [], [], [], []
        self.gru = (mix(7), 0, False)
        self.lstm = (mix(11), 0, False)
        self.pose_prev = (mix(13), 0, False)
        self.head_rows = 0
        self.emitted = []                # ("mouth" | "pose", index, value, read_end, padded)

    @staticmethod
    def fold(a, b):
        return (mix(a[0], b[0]), max(a[1], b[1]), a[2] or b[2])

    def feed(self, samples, first, keep_from):
        assert first == self.n and len(samples) > 0
        assert keep_from >= self.kept_from
        self.kept_from = keep_from
        self.n += len(samples)

    def mel(self, w0, w1, ended):
        assert w0 == len(self.mel_rows)
        for i in range(w0, w1):
            st = window_start(i)
            assert st >= self.kept_from, "window %d reads samples dropped from the buffer" % i
            end = st + 266
            padded = end > self.n
            assert not padded or ended, "window %d zero padded before the end of the clip" % i
            self.mel_rows.append((mix(1, i, st, min(end, self.n), padded), min(end, self.n), padded))

    def apc(self, w0, w1):
        assert w0 == len(self.apc_rows) and w1 <= len(self.mel_rows)
        for j in range(w0, w1):
            self.gru = self.fold(self.gru, self.mel_rows[j])
            self.apc_rows.append(self.gru)

    def lle(self, w0, w1):
        assert w0 == len(self.lle_rows) and w1 <= len(self.apc_rows)
        for j in range(w0, w1):
            a = self.apc_rows[j]
            self.lle_rows.append((mix(2, a[0]), a[1], a[2]))

    def pairs(self, p0, p1):
        assert p0 == len(self.pair_rows) and 2 * p1 <= len(self.lle_rows)
        for p in range(p0, p1):
            self.pair_rows.append(self.fold(self.lle_rows[2 * p], self.lle_rows[2 * p + 1]))

    def mouth(self, steps, npairs, frames):
        a0, a1 = steps
        m0, m1 = frames
        assert npairs == len(self.pair_rows)
        outs = {}
        for k in range(a0, a1):
            if k < npairs:
                row = self.pair_rows[k]
            else:
                assert self.sched.ended, "tail step before finish()"
                last = self.lle_rows[-1]
                row = (mix(3, last[0]), last[1], last[2])
            self.lstm = self.fold(self.lstm, row)
            outs[k] = self.lstm
        for t in range(m0, m1):
            v = outs[t + FF_MOUTH]
            self.emitted.append(("mouth", t) + v)

    def poses(self, rows, frames):
        r0, r1 = rows
        assert r0 == self.head_rows and r1 <= len(self.pair_rows)
        self.head_rows = r1
        for i in range(*frames):
            assert i + FF_HEAD < self.head_rows, "pose %d before its pair row was handed over" % i
            self.pose_prev = self.fold(self.pose_prev, self.pair_rows[i + FF_HEAD])
            self.emitted.append(("pose", i) + self.pose_prev)


def run(pieces, max_chunk=16000):
    s = LiveScheduler(FF_MOUTH, FF_HEAD, max_chunk)
    b = ProvenanceBackend(s)
    pushed = 0
    for k in pieces:
        before = len(b.emitted)
        for plan in s.plan_push(k):
            run_plan(b, plan, np.zeros(plan.samples[1] - plan.samples[0], np.float32))
        pushed += k
        for item in b.emitted[before:]:
            assert item[3] <= pushed and not item[4], "%s %d emitted before all its samples were pushed" % item[:2]
    run_plan(b, s.plan_finish(), None)
    with pytest.raises(RuntimeError):
        s.plan_push(1)
    return b.emitted, pushed


def by_kind(emitted):
    """mouth rows and poses are two streams: each in order, each item once (how they interleave depends on the chunking)"""
    return [e for e in emitted if e[0] == "mouth"], [e for e in emitted if e[0] == "pose"]


def check_counts(emitted, N):
    n = num_frames(N)
    mouth = [e[1] for e in emitted if e[0] == "mouth"]
    poses = [e[1] for e in emitted if e[0] == "pose"]
    assert mouth == list(range(n)) and poses == list(range(max(n - FF_HEAD, 0)))


def test_chunkings_equal_single_push_and_are_causal():
    rng = np.random.default_rng(2024)
    for trial in range(2000):
        N = int(rng.integers(0, 40001))
        ref, _ = run([N] if N else [])
        check_counts(ref, N)
        style = trial % 4
        pieces, left = [], N
        while left > 0:
            if style == 0:
                k = int(rng.integers(1, 8001))
            elif style == 1:
                k = int(rng.integers(1, 300))
            elif style == 2:
                k = 266 + int(rng.integers(0, 2))
            else:
                k = int(rng.choice([1, 2, 133, 134, 5000, 20000]))
            k = min(k, left)
            pieces.append(k)
            left -= k
        if trial % 5 == 0:
            pieces.insert(int(rng.integers(0, len(pieces) + 1)), 0)          # empty pushes change nothing
        got, pushed = run(pieces, max_chunk=int(rng.choice([1000, 4000, 16000])))
        assert pushed == N
        assert by_kind(got) == by_kind(ref), "trial %d: N %d pieces %s" % (trial, N, pieces[:10])


@pytest.mark.parametrize("N", [0, 266, 267, 399, 5000, 12000])
def test_one_sample_pushes(N):
    ref, _ = run([N] if N else [])
    got, _ = run([1] * N)
    assert by_kind(got) == by_kind(ref)
    check_counts(got, N)


def test_empty_clip_and_shorter_than_lookaheads():
    for N in (0, 1, 100, 266):
        got, _ = run([N])
        assert got == []
    # one frame: no pose, its mouth row only at finish
    s = LiveScheduler(FF_MOUTH, FF_HEAD, 16000)
    assert [p.mouth for p in s.plan_push(267)] == [(0, 0)]
    assert s.plan_finish().mouth == (0, 1)
    # 16 frames (between both lookaheads): one pose, every mouth row at finish
    N = 16 * 16000 // 60 + 1
    s = LiveScheduler(FF_MOUTH, FF_HEAD, 16000)
    plans = s.plan_push(N)
    assert plans[-1].mouth == (0, 0)
    fin = s.plan_finish()
    assert fin.mouth == (0, 16) and (plans[-1].poses[1], fin.poses[1]) == (0, 1)


def test_final_window_rule():
    """The rule of the issue, checked directly: window i final iff i < 2*int(N/16000*60) and its clip lies inside the N samples;
    a final window is one the finished clip has; at most 2 samples of wait past full coverage."""
    for N in range(0, 60000, 7):
        W = final_windows(N, False)
        total = 2 * num_frames(N)
        assert W <= total
        for i in (W - 1, W):
            if 0 <= i < total:
                assert (window_start(i) + 266 <= N) == (i < W)
        assert W == final_windows(N, True) or window_start(W) + 266 > N or W == total
    for i in range(1, 5000):
        covered = window_start(i) + 266
        assert final_windows(covered + 2, False) > i


def test_lookahead_numbers():
    """Derived trailing distances quoted in live.py / DESIGN.md: samples from the start of a frame until it can be emitted."""
    def first_n(pred):
        lo, hi = 0, 10 ** 7
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if pred(mid) else (mid + 1, hi)
        return lo
    t = 300
    start = int(t * 16000 / 60)
    mouth = first_n(lambda N: max(0, final_windows(N, False) // 2 - FF_MOUTH) > t) - start
    pose = first_n(lambda N: max(0, final_windows(N, False) // 2 - FF_HEAD) > t) - start
    print("\n[live] mouth frame trails its start by %d samples, head pose by %d" % (mouth, pose))
    assert 5100 <= mouth <= 5300 and 4300 <= pose <= 4500


def test_headers_declare_the_live_entry_points():
    want = {"lsprnn.h": ("lsprnn_forward_state", "lsprnn_state_floats"),
            "lspa2h.h": ("lspa2h_generate_resume", "lspa2h_state_bytes"),
            "lspmel.h": ("lspmel_compute_range", "lspmel_window_start")}
    for hdr, names in want.items():
        text = open(os.path.join(ROOT, "include", hdr)).read()
        for n in names:
            assert re.search(r"\b%s\s*\(" % n, text), (hdr, n)
    from livespeechportraits_amd import _native as N
    lib = ctypes.CDLL(N.LIB_PATH)
    for names in want.values():
        for n in names:
            assert hasattr(lib, n)


def test_window_start_matches_the_library():
    from livespeechportraits_amd import _native as N
    lib = N.load()
    for i in list(range(0, 3000)) + [10 ** 6 + 7, 12345678]:
        assert lib.lspmel_window_start(i) == window_start(i)
    for n in list(range(0, 2000, 3)) + [183200, 400000, 399999]:
        assert lib.lspmel_num_windows(n) == 2 * num_frames(n)


def test_session_refuses_cpu_device():
    from livespeechportraits_amd.live import LiveAudioFrontEnd
    with pytest.raises(RuntimeError, match="GPU"):
        LiveAudioFrontEnd(None, None, None, None, True, 10, 1.0, np.zeros(12, np.float32), 0.3, device="cpu")
