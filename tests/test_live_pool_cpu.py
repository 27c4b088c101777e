"""CPU tests of the live session pool's host side (livespeechportraits_amd/live_pool.py: PoolPlanner, run_pool_round) and of the
priming planner (live.py: PrimingPlanner), with the provenance backend of tests/test_live_cpu.py: one per session, behind a pool backend
that counts how often each stage is called."""
import ctypes
import os
import re

import numpy as np
import pytest

from livespeechportraits_amd.live import LiveScheduler, PrimingPlanner, run_plan
from livespeechportraits_amd.live_pool import MAX_SESSIONS, PoolPlanner, run_pool_round
from test_live_cpu import FF_HEAD, FF_MOUTH, ProvenanceBackend, by_kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD = 255


class PoolBackend:
    """run_pool_round's backend: every stage takes a list of (session, ...) and hands each entry to that session's ProvenanceBackend."""

    def __init__(self):
        self.b = {}
        self.calls = {}

    def _each(self, stage, items):
        self.calls[stage] = self.calls.get(stage, 0) + 1
        keys = [it[0] for it in items]
        assert keys == sorted(set(keys)) and items, "a stage lists each session once, in ascending order, and is not called for nobody"
        for it in items:
            getattr(self.b[it[0]], stage)(*it[1:])

    def feed(self, items):
        self._each("feed", items)

    def mel(self, items):
        self._each("mel", items)

    def apc(self, items):
        self._each("apc", items)

    def lle(self, items):
        self._each("lle", items)

    def pairs(self, items):
        self._each("pairs", items)

    def mouth(self, items):
        self._each("mouth", items)

    def poses(self, items):
        self.calls["poses"] = self.calls.get("poses", 0) + 1
        for sid, rows, steps, frames in items:
            assert steps[1] > steps[0]
            self.b[sid].poses(rows, frames)


def alone(pushes, finished, max_chunk):
    """What a LiveScheduler of its own emits for the same pushes (no finish: the session was closed, or still runs)."""
    s = LiveScheduler(FF_MOUTH, FF_HEAD, max_chunk)
    b = ProvenanceBackend(s)
    for k in pushes:
        for plan in s.plan_push(k):
            run_plan(b, plan, np.zeros(plan.samples[1] - plan.samples[0], np.float32))
    if finished:
        run_plan(b, s.plan_finish(), None)
    return b.emitted


def test_pool_sessions_equal_schedulers_of_their_own():
    rng = np.random.default_rng(77)
    for trial in range(60):
        max_sessions = int(rng.integers(1, MAX_SESSIONS + 1))
        max_chunk = int(rng.choice([1000, 4000, 16000]))
        pool = PoolPlanner(max_sessions, FF_MOUTH, FF_HEAD, FIELD, max_chunk, int(rng.choice([1, 16, 254])))
        be = PoolBackend()
        pushes, done = {}, {}                                                  # sid -> pushes so far; sid -> (emitted, pushes, finished)
        for tick in range(int(rng.integers(5, 60))):
            while len(pool.slot) < max_sessions and rng.random() < 0.3:        # sessions open at different ticks, in freed slots too
                sid = pool.open()
                assert sid not in pushes and sid not in done
                be.b[sid] = ProvenanceBackend(pool.sched[sid])
                pushes[sid] = []
            if len(pool.slot) == max_sessions:
                with pytest.raises(RuntimeError, match="max_sessions"):
                    pool.open()
            lengths, finish = {}, set()
            for sid in list(pool.slot):
                r = rng.random()
                if r < 0.15:
                    continue                                                   # not in this tick
                k = int(rng.choice([0, 1, 266, 267, int(rng.integers(1, 300)), int(rng.integers(1000, 9000))]))
                if r < 0.9:
                    lengths[sid] = k
                if rng.random() < 0.06:
                    finish.add(sid)
            be.calls = {}
            rounds = pool.rounds(lengths, finish)
            for work in rounds:
                be.calls = {}
                run_pool_round(be, [(sid, p, np.zeros(n, np.float32) if n else None, rows, steps) for sid, p, (o, n), rows, steps in work])
                assert all(c == 1 for c in be.calls.values()), "a stage was called more than once in a round: %s" % be.calls
            want_rounds = max([len(range(0, lengths.get(sid, 0), max_chunk)) + (sid in finish) for sid in set(lengths) | finish], default=0)
            assert len(rounds) == want_rounds
            for sid, k in lengths.items():
                pushes[sid].append(k)
            for sid in finish:
                done[sid] = (be.b[sid].emitted, pushes.pop(sid), True)
                pool.close(sid)
                with pytest.raises(RuntimeError, match="closed"):
                    pool.check(sid)
            if pool.slot and rng.random() < 0.05:                              # closed without finish
                sid = sorted(pool.slot)[0]
                done[sid] = (be.b[sid].emitted, pushes.pop(sid), False)
                pool.close(sid)
        for sid, p in pushes.items():
            done[sid] = (be.b[sid].emitted, p, False)
        for sid, (emitted, p, finished) in done.items():
            assert by_kind(emitted) == by_kind(alone(p, finished, max_chunk)), "trial %d session %d" % (trial, sid)
        assert sorted(pool.free + list(pool.slot.values())) == list(range(max_sessions))


def test_pool_planner_refusals():
    with pytest.raises(ValueError):
        PoolPlanner(0, FF_MOUTH, FF_HEAD, FIELD, 16000, 16)
    with pytest.raises(ValueError):
        PoolPlanner(MAX_SESSIONS + 1, FF_MOUTH, FF_HEAD, FIELD, 16000, 16)
    with pytest.raises(ValueError):
        PoolPlanner(4, FF_MOUTH, FF_HEAD, FIELD, 16000, 0)
    pool = PoolPlanner(2, FF_MOUTH, FF_HEAD, FIELD, 16000, 16)
    a, b = pool.open(), pool.open()
    assert (pool.slot[a], pool.slot[b]) == (0, 1)
    with pytest.raises(RuntimeError, match="max_sessions"):
        pool.open()
    with pytest.raises(KeyError):
        pool.check(99)
    with pytest.raises(KeyError):
        pool.check("x")
    pool.close(a)
    with pytest.raises(RuntimeError, match="closed"):
        pool.check(a)
    c = pool.open()
    assert c not in (a, b) and pool.slot[c] == 0                             # a new id in the freed slot


# ---- the priming planner ---------------------------------------------------------------------------------------------------
def _drive(field, ff, per_tick, pieces, max_chunk=16000):
    """One session fed `pieces` (one tick each): -> per round (tick, npairs, rows, steps, poses), and the ring rows the planner asks for."""
    sched = LiveScheduler(FF_MOUTH, ff, max_chunk)
    prime = PrimingPlanner(field, ff, per_tick)
    log = []
    for tick, k in enumerate(pieces):
        prime.begin_tick()
        plans = sched.plan_push(k) if k >= 0 else [sched.plan_finish()]
        for p in plans:
            rows, steps = prime.plan(p.pairs[1], p.poses)
            log.append((tick, p.pairs[1], rows, steps, p.poses, p.pairs[1] - p.pairs[0]))
    return log


@pytest.mark.parametrize("field,ff", [(255, 15), (16, 3)])                   # the shipped WaveNet; the small golden case a2h_nc2_l4b1
@pytest.mark.parametrize("per_tick", [1, 16, 254])
def test_priming_planner(field, ff, per_tick):
    f1 = field - 1
    rng = np.random.default_rng(field + per_tick)
    frame = lambda: 266 + int(rng.integers(0, 2))
    ways = {"per_frame": [frame() for _ in range(400)] + [-1],
            "whole": [120000, -1],
            "small_then_frames": [1] * 400 + [frame() for _ in range(300)] + [-1],
            "random": [int(rng.integers(1, 8000)) for _ in range(60)] + [-1],
            "short_clip": [frame() for _ in range(ff + 3)] + [-1],
            "chunked": [50000, 3000, -1]}
    for name, pieces in ways.items():
        max_chunk = 2000 if name == "chunked" else 16000
        log = _drive(field, ff, per_tick, pieces, max_chunk)
        max_pairs = max(e[5] for e in log)
        ring = PrimingPlanner.ring_rows_needed(ff, max_pairs)
        next_step, handed, per_tick_steps, frame_tick = 0, 0, {}, {}
        for tick, npairs, (r0, r1), (s0, s1), (h0, h1), _ in log:
            assert s0 == next_step and s1 >= s0, "%s: steps in order, each once" % name
            next_step = s1
            assert r0 == handed and r1 >= r0 and r1 <= npairs and (r1 == r0 or s1 > s0), "%s: rows handed once, only with steps" % name
            handed = r1
            if h1 > h0:
                frame_tick[tick] = True
                assert s1 == f1 + h1 and (s0 == f1 + h0 or (h0 == 0 and s0 <= f1)), "%s: all priming done before pose 0, poses in step" % name
            else:
                assert s1 == s0 or s1 <= f1, "%s: a pose step without a pose due" % name
            for s in range(s0, s1):
                row = max(0, s + ff - f1)
                assert row < handed, "%s: step %d before pair row %d was known" % (name, s, row)
                assert row >= handed - ring, "%s: pair row %d left a ring of %d rows before step %d read it" % (name, row, ring, s)
            per_tick_steps[tick] = per_tick_steps.get(tick, 0) + sum(1 for s in range(s0, s1) if s < f1)
        for tick, n in per_tick_steps.items():
            assert n <= per_tick or frame_tick.get(tick), "%s: %d priming steps in tick %d" % (name, n, tick)
        total_poses = log[-1][4][1]
        assert next_step == (f1 + total_poses if total_poses else next_step) and (total_poses == 0 or next_step >= f1)
        if name == "per_frame" and per_tick >= 16:
            # the point of the slices: from the first pair row on there are ff ticks before pose 0, enough for every step that reads row 0
            first_pose_tick = min(frame_tick)
            assert per_tick_steps[first_pose_tick] <= max(per_tick, ff), "%s: priming left for the tick of pose 0: %d steps" % (name, per_tick_steps[first_pose_tick])
    # LiveSessionPool's ring (max_pairs + ff + 1 rows) is long enough
    assert PrimingPlanner.ring_rows_needed(ff, 10) <= 10 + ff + 1
    with pytest.raises(ValueError):
        PrimingPlanner(field, ff, 0)


def test_headers_declare_the_pool_entry_points():
    want = {"lsprnn.h": ("lsprnn_forward_multi",),
            "lspa2h.h": ("lspa2h_generate_resume_multi", "lspa2h_workspace_bytes_multi", "lspa2h_bind_workspace_multi", "lspa2h_status_multi"),
            "lspmel.h": ("lspmel_compute_ranges",)}
    from livespeechportraits_amd import _native as N
    lib = ctypes.CDLL(N.LIB_PATH)
    for hdr, names in want.items():
        text = open(os.path.join(ROOT, "include", hdr)).read()
        for n in names:
            assert re.search(r"\b%s\s*\(" % n, text), (hdr, n)
            assert hasattr(lib, n)


def test_pool_refuses_cpu_device():
    from livespeechportraits_amd.live_pool import LiveSessionPool
    with pytest.raises(RuntimeError, match="GPU"):
        LiveSessionPool(None, None, None, None, True, 10, 1.0, device="cpu")
