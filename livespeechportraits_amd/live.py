"""Live audio front-end: the audio half of demo.py (mel -> APC GRU encoder -> KNN + LLE -> Audio2Feature LSTM and the head-pose
WaveNet, demo.py:183-216) fed with audio as it arrives instead of a whole clip.

Every network of that chain is causal apart from a fixed lookahead, so a chunked run gives the bits of the whole-clip run: the GRU and
LSTM carry their state between calls (lsprnn_forward_state), the WaveNet carries its dilation queues (lspa2h_generate_resume), the mel
front-end computes a window range (lspmel_compute_range), and every row-wise stage reduces in an order that does not depend on how many
rows a call has.  What becomes final when is decided by ``LiveScheduler``, and when the head-pose WaveNet's priming steps run by
``PrimingPlanner``: both pure Python with no device code (``run_plan`` drives a provenance fake with their plans in tests/test_live_cpu.py).  The
device side is written once, in live_pool.py: ``LiveSessionPool`` runs the stages for 1..16 streams per call, and
``LiveAudioFrontEnd`` here is the one session of a pool of one, so priming is spread over the pushes for it too.

Lookahead, derived from the finality rules (DESIGN.md "Live audio"): mouth frame t needs pair row t + 18, i.e. mel window 2t + 37,
whose clip ends at sample int((2t + 37) * 133.33) + 266 -- about 5 200 samples (325 ms) after the start of frame t (t * 266.67);
head pose i needs pair row i + 15, window 2i + 31: about 4 400 samples (275 ms)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, NamedTuple

SAMPLE_RATE = 16000
MEL_WIN = 266                          # int(16000 / 60): the clip of one mel window
MEL_STEP = SAMPLE_RATE * (0.5 / 60)    # mel_frame_step of utils.py:70, the same double


def window_start(i: int) -> int:
    """int(i * mel_frame_step) (utils.py:74): the first sample of mel window i."""
    return int(i * MEL_STEP)


def num_frames(nsamples: int) -> int:
    """int(N / 16000 * 60): video frames of a clip of N samples (demo.py:179; lspmel_num_windows is twice this)."""
    return int(nsamples / 16000 * 60)


def final_windows(nsamples: int, ended: bool) -> int:
    """Mel windows that are final after N samples: window i once i < 2 * int(N / 16000 * 60) and its 266-sample clip lies inside
    the samples pushed; at the end of the clip every window, the last ones zero padded."""
    total = 2 * num_frames(nsamples)
    if ended or total == 0:
        return total
    if nsamples < MEL_WIN:
        return 0
    c = min(total, int((nsamples - MEL_WIN) / MEL_STEP) + 2)
    while c > 0 and window_start(c - 1) + MEL_WIN > nsamples:
        c -= 1
    return c


@dataclass
class LivePlan:
    """One step of work.  Ranges are [start, stop) in stream indices."""
    samples: tuple        # new samples of the stream in this step
    ended: bool           # the clip ends after them (finish())
    windows: tuple        # mel windows == APC rows == LLE rows
    pairs: tuple          # pair rows (LLE rows 2p, 2p+1): the 1024-wide rows both downstream models read
    a2f_steps: tuple      # Audio2Feature LSTM steps; steps >= the number of pair rows are the tail (last LLE row repeated)
    mouth: tuple          # mouth frames emitted: LSTM steps [mouth + frame_future]
    head_rows: tuple      # pair rows handed to the head-pose generator in this step (passed once, when poses follow)
    poses: tuple          # head poses emitted


class LiveScheduler:
    """When each item becomes final (the reference's own index arithmetic; DESIGN.md "Live audio"):

    ============  ==============================================================================================
    mel window i  i < 2 * int(N / 16000 * 60) and int(i * 133.33..) + 266 <= N  (all of them at finish)
    APC / LLE j   mel window j is final
    mouth t       pair row t + ff_mouth exists (LLE rows up to 2(t + ff_mouth) + 1); the tail only at finish
    head pose i   pair row i + ff_head exists, and i < n - ff_head
    ============  ==============================================================================================

    N is the number of samples pushed so far, n = int(N / 16000 * 60) the clip's frames at finish.  Totals: n mouth frames,
    max(n - ff_head, 0) head poses."""

    def __init__(self, ff_mouth: int = 18, ff_head: int = 15, max_chunk_samples: int = 16000):
        if ff_mouth < 0 or ff_head < 0 or max_chunk_samples < 1:
            raise ValueError("frame_future values must be >= 0 and max_chunk_samples >= 1")
        self.ff_mouth, self.ff_head, self.max_chunk = ff_mouth, ff_head, max_chunk_samples
        self.n_samples = 0
        self.ended = False
        self.w = self.p = self.a = self.m = self.r = self.h = 0

    def _step(self, n_new: int, ended: bool) -> LivePlan:
        s0 = self.n_samples
        N = s0 + n_new
        W = final_windows(N, ended)
        P = W // 2
        if ended:
            n = num_frames(N)
            A = n + self.ff_mouth if n > 0 else 0
        else:
            A = P
        M = max(0, A - self.ff_mouth)
        H = max(0, P - self.ff_head)
        R = P if H > self.h else self.r
        plan = LivePlan((s0, N), ended, (self.w, W), (self.p, P), (self.a, A), (self.m, M), (self.r, R), (self.h, H))
        self.n_samples, self.ended = N, ended
        self.w, self.p, self.a, self.m, self.r, self.h = W, P, A, M, R, H
        return plan

    def plan_push(self, n: int) -> List[LivePlan]:
        """Plans for n more samples, split into steps of at most max_chunk_samples."""
        if self.ended:
            raise RuntimeError("the clip has ended (finish() was called): no more audio can be pushed")
        if n < 0:
            raise ValueError("negative sample count")
        plans = []
        while n > 0:
            k = min(n, self.max_chunk)
            plans.append(self._step(k, False))
            n -= k
        return plans

    def plan_finish(self) -> LivePlan:
        if self.ended:
            raise RuntimeError("finish() was already called")
        return self._step(0, True)


class PrimingPlanner:
    """Which steps of the head-pose WaveNet a session runs in each step of work, when the field - 1 priming steps before pose 0 are
    spread over the ticks instead of run in one go (LiveSessionPool; lspa2h_generate_resume_multi takes step ranges).

    Step s < field - 1 primes and emits nothing, step field - 1 + i emits pose i; step s reads pair row max(0, s + ff_head - (field - 1)).
    Rules: a step runs only once the row it reads exists; while no pose is due a session runs at most ``prime_steps_per_tick`` priming
    steps per tick (``begin_tick`` refills the budget); when poses are due, every step up to the last of them runs at once, whatever
    is left of the priming included (a whole clip pushed at once primes in one go).  Pair rows are handed to the generator when steps
    run, all that exist: until pose 0 the rows 0..ff_head must stay in the generator's ring, which therefore holds at least
    ff_head + (pair rows one step of work can add) rows -- ``ring_rows_needed``."""

    def __init__(self, field: int, ff_head: int, prime_steps_per_tick: int = 16):
        if field < 1 or ff_head < 0 or prime_steps_per_tick < 1:
            raise ValueError("need field >= 1, frame_future >= 0 and prime_steps_per_tick >= 1")
        self.f1, self.ff, self.per_tick = field - 1, ff_head, prime_steps_per_tick
        self.step = 0          # the next step
        self.rows = 0          # pair rows handed to the generator
        self.budget = prime_steps_per_tick

    @staticmethod
    def ring_rows_needed(ff_head: int, max_pairs_per_step: int) -> int:
        return ff_head + max_pairs_per_step

    def begin_tick(self) -> None:
        self.budget = self.per_tick

    def plan(self, npairs: int, poses) -> tuple:
        """One step of work: ``npairs`` pair rows exist, ``poses`` = (h0, h1) are due (LivePlan.poses).  -> ((r0, r1), (s0, s1)): pair rows
        to hand over and steps to run; r1 > r0 only when s1 > s0."""
        h0, h1 = poses
        s0 = self.step
        if h1 > h0:
            if s0 > self.f1 + h0 or (s0 < self.f1 + h0 and h0 > 0):
                raise RuntimeError("internal: head-pose steps out of step with the poses due")
            s1 = self.f1 + h1
        elif s0 < self.f1 and npairs > 0:
            s1 = max(s0, min(self.f1, s0 + self.budget, npairs + self.f1 - self.ff))
            self.budget -= s1 - s0
        else:
            s1 = s0
        r0 = self.rows
        r1 = npairs if s1 > s0 else r0
        self.step, self.rows = s1, r1
        return (r0, r1), (s0, s1)


def run_plan(backend, plan: LivePlan, samples) -> None:
    """The order every step of ONE session runs in, stated without a device; ``backend`` provides the stages.  The device runs
    live_pool.run_pool_round, the same order for several sessions, and is held to this statement by tests/test_live_pool_cpu.py
    (a provenance double behind both):
    feed(samples, first_sample, keep_from)  append the new samples; samples before `keep_from` are no longer read
    mel(w0, w1, ended) / apc(w0, w1) / lle(w0, w1)   windows == rows [w0, w1)
    pairs(p0, p1)                            pair rows [p0, p1) from LLE rows [2 p0, 2 p1)
    mouth(steps, npairs, frames)             Audio2Feature steps [a0, a1) (>= npairs: the tail); emit mouth frames [m0, m1)
    poses(rows, frames)                      hand pair rows [r0, r1) to the head-pose generator; emit poses [h0, h1)"""
    if plan.samples[1] > plan.samples[0]:
        backend.feed(samples, plan.samples[0], window_start(plan.windows[0]))
    if plan.windows[1] > plan.windows[0]:
        backend.mel(plan.windows[0], plan.windows[1], plan.ended)
        backend.apc(plan.windows[0], plan.windows[1])
        backend.lle(plan.windows[0], plan.windows[1])
    if plan.pairs[1] > plan.pairs[0]:
        backend.pairs(plan.pairs[0], plan.pairs[1])
    if plan.a2f_steps[1] > plan.a2f_steps[0]:
        backend.mouth(plan.a2f_steps, plan.pairs[1], plan.mouth)
    if plan.poses[1] > plan.poses[0]:
        backend.poses(plan.head_rows, plan.poses)


# ------------------------------------------------------------------------------------------------------------ device session
class LiveFrames(NamedTuple):
    """Frames that became final in one push()/finish(): mouth rows [k_f, 75] (mouth_start = index of the first), head poses
    [k_h, ndim] (pose_start likewise).  Device tensors; numpy arrays when the call asked for a host copy."""
    mouth: object
    mouth_start: int
    poses: object
    pose_start: int


class LiveAudioFrontEnd:
    """demo.py's audio stages for one stream of audio that arrives in pieces, on the device: the one session of a LiveSessionPool of one
    (live_pool.py, which holds the stages, the carried state and the device memory -- there is no second implementation here).

    Built from what demo.py:146-166 builds and reads from the config: the APC_encoder, the Audio2FeatureModel and the
    Audio2HeadposeModel (the drop-ins of this package), APC_feat_database, use_LLE, Knear, LLE_percent, pre_headpose, sigma_scale, and
    both frame_future values (taken from the option objects: ``feature_opt`` / ``headpose_opt``, default the models' own ``opt``).
    ``push(samples)`` returns the frames that became final; ``finish()`` flushes the end of the clip, after which the stream has ended
    for good (a pool session's slot can be reopened; this object cannot).  Pushed in any pieces, the outputs are bit for bit those of
    the whole-clip path (mel.compute_mel -> APC_encoder -> manifold.project -> generate_sequences).  GMM noise is drawn per head-pose
    frame, in frame order, from ``generator`` (default: the global one) in draw_gmm_noise's order.  Everything else -- fixed device
    memory, pushes longer than ``max_chunk_samples``, the head-pose priming spread ``prime_steps_per_tick`` steps per push, the status
    words -- is LiveSessionPool's, and is described there.  So are the refusals of the constructor and of the samples: they are
    raised by the pool and name it (and the session, 0) in their messages."""

    def __init__(self, APC_model, Audio2Feature, Audio2Headpose, APC_feat_database, use_LLE: bool, Knear: int, LLE_percent: float,
                 pre_headpose, sigma_scale: float, device="cuda:0", max_chunk_samples: int = 16000, feature_opt=None, headpose_opt=None,
                 generator=None, prime_steps_per_tick: int = 16):
        from .live_pool import LiveSessionPool
        self.pool = LiveSessionPool(APC_model, Audio2Feature, Audio2Headpose, APC_feat_database, use_LLE, Knear, LLE_percent,
                                    sigma_scale=sigma_scale, device=device, max_sessions=1, max_chunk_samples=max_chunk_samples,
                                    feature_opt=feature_opt, headpose_opt=headpose_opt, prime_steps_per_tick=prime_steps_per_tick)
        self.sid = self.pool.open(pre_headpose, generator)
        self.ff_mouth, self.ff_head = self.pool.ff_mouth, self.pool.ff_head
        self.sched = self.pool.plan.sched[self.sid]                              # held here: it outlives the close that finish() causes
        self.ended = False

    def push(self, samples, host: bool = False) -> LiveFrames:
        """Take float32 16 kHz samples (host array or device tensor, any length); return the frames that became final."""
        if self.ended:
            raise RuntimeError("the clip has ended (finish() was called): no more audio can be pushed")
        return self.pool.tick({self.sid: samples}, host=host)[self.sid]

    def finish(self, host: bool = False) -> LiveFrames:
        """End of the clip: the zero-padded last windows, the Audio2Feature tail and the remaining head poses."""
        if self.ended:
            raise RuntimeError("finish() was already called")
        self.ended = True
        return self.pool.tick(finish=[self.sid], host=host)[self.sid]
