"""Live audio front-end: the audio half of demo.py (mel -> APC GRU encoder -> KNN + LLE -> Audio2Feature LSTM and the head-pose
WaveNet, demo.py:183-216) fed with audio as it arrives instead of a whole clip.

Every network of that chain is causal apart from a fixed lookahead, so a chunked run gives the bits of the whole-clip run: the GRU and
LSTM carry their state between calls (lsprnn_forward_state), the WaveNet carries its dilation queues (lspa2h_generate_resume), the mel
front-end computes a window range (lspmel_compute_range), and every row-wise stage reduces in an order that does not depend on how many
rows a call has.  What becomes final when is decided by ``LiveScheduler``, pure Python with no device code; ``run_plan`` drives any
backend with its plans (``LiveAudioFrontEnd`` on the device, a provenance fake in tests/test_live_cpu.py).

Lookahead, derived from the finality rules (DESIGN.md "Live audio"): mouth frame t needs pair row t + 18, i.e. mel window 2t + 37,
whose clip ends at sample int((2t + 37) * 133.33) + 266 -- about 5 200 samples (325 ms) after the start of frame t (t * 266.67);
head pose i needs pair row i + 15, window 2i + 31: about 4 400 samples (275 ms)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, NamedTuple

import numpy as np

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
    ff_head + (pair rows one step of work can add) rows -- ``ring_rows_needed``; LiveAudioFrontEnd's ring is one row longer."""

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
    """The order every step runs in; ``backend`` provides the stages (LiveAudioFrontEnd, or a test double):
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
    """demo.py's audio stages for audio that arrives in pieces, on the device.

    Built from what demo.py:146-166 builds and reads from the config: the APC_encoder, the Audio2FeatureModel and the
    Audio2HeadposeModel (the drop-ins of this package), APC_feat_database, use_LLE, Knear, LLE_percent, pre_headpose, sigma_scale, and
    both frame_future values (taken from the option objects: ``feature_opt`` / ``headpose_opt``, default the models' own ``opt``).
    ``push(samples)`` returns the frames that became final; ``finish()`` flushes the end of the clip.  Pushed in any pieces, the
    outputs are bit for bit those of the whole-clip path (mel.compute_mel -> APC_encoder -> manifold.project -> generate_sequences).
    GMM noise is drawn per head-pose frame, in frame order, from ``generator`` (default: the global one) in draw_gmm_noise's order.
    Device memory is fixed at construction; a push longer than ``max_chunk_samples`` is split internally.  The status words are read
    once per push; a lost inter-workgroup hand-off (another stream holding the CUs for the whole time-out) ends the session with an error.
    Every stage keeps its input state in a buffer of its own (two per stage, used in turn), so a caller that drives the C entry points
    directly can run a failed call again from the same state."""

    def __init__(self, APC_model, Audio2Feature, Audio2Headpose, APC_feat_database, use_LLE: bool, Knear: int, LLE_percent: float,
                 pre_headpose, sigma_scale: float, device="cuda:0", max_chunk_samples: int = 16000, feature_opt=None, headpose_opt=None,
                 generator=None):
        import torch
        self.torch = torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("LiveAudioFrontEnd runs on the MI355X only: device must be a GPU (there is no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if getattr(APC_model, "rnn_residual", False):
            raise NotImplementedError("residual APC stacks are not supported (no shipped config enables them)")
        fo = feature_opt if feature_opt is not None else Audio2Feature.opt
        ho = headpose_opt if headpose_opt is not None else Audio2Headpose.opt
        if getattr(ho, "feature_decoder", "WaveNet") != "WaveNet":
            raise NotImplementedError("the live path generates head poses with the WaveNet decoder only (the LSTM decoder is in no shipped config)")
        if max_chunk_samples < 1:
            raise ValueError("max_chunk_samples must be >= 1")
        self.device = dev
        self.ff_mouth, self.ff_head = int(fo.frame_future), int(ho.frame_future)
        self.sched = LiveScheduler(self.ff_mouth, self.ff_head, max_chunk_samples)
        self.use_lle, self.knear, self.lle_percent = bool(use_LLE), int(Knear), float(LLE_percent)
        self.sigma_scale = float(sigma_scale)
        self.generator = generator
        self.nd, self.nc, self.gmm = int(ho.A2H_GMM_ndim), int(ho.A2H_GMM_ncenter), ho.loss == "GMM"
        f32 = dict(dtype=torch.float32, device=dev)
        # the stages' engines (built, bound and sized here, once)
        max_win = 2 * (max_chunk_samples // MEL_WIN + 2) + 2                   # windows that one step can make final
        max_pairs = max_win // 2 + 1
        self.apc_eng = APC_model._get_engine(dev, max_win)
        a2f = Audio2Feature.Audio2Feature
        a2f = a2f.module if hasattr(a2f, "module") else a2f
        self.a2f_pk = a2f._pack(dev, max_pairs + self.ff_mouth)
        net = Audio2Headpose._net()
        # a head-pose engine of its own: its workspace is this session's projection ring (whole-clip calls would overwrite a shared one)
        from .a2h_engine import HeadposeEngine
        o = net.opt
        self.a2h_eng = HeadposeEngine(o.A2H_wavenet_residual_layers, o.A2H_wavenet_residual_blocks, o.A2H_wavenet_residual_channels,
                                  o.A2H_wavenet_dilation_channels, o.A2H_wavenet_skip_channels, o.A2H_wavenet_kernel_size,
                                  o.A2H_wavenet_input_channels, o.A2H_wavenet_cond_channels, o.APC_hidden_size,
                                  o.A2H_GMM_ncenter, o.A2H_GMM_ndim, o.loss, max_audio_frames=max_pairs + self.ff_head + 1)
        self.a2h_eng.load_state_dict({k: v for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")})
        self.a2h_eng.bind(dev)
        self.db = torch.as_tensor(np.ascontiguousarray(APC_feat_database, np.float32)).to(dev) if self.use_lle else None
        self.pre = torch.as_tensor(np.ascontiguousarray(np.asarray(pre_headpose, np.float32).reshape(-1))).to(dev)
        from . import _native as N
        lib = N.load()
        self.mel_ws = torch.empty(int(lib.lspmel_workspace_bytes(max_win)), dtype=torch.uint8, device=dev)
        self.scap = max_chunk_samples + 4 * MEL_WIN                              # samples not yet consumed + one step
        self.sbuf = torch.empty(self.scap, **f32)
        self.sbase = self.slen = 0                                               # sbuf[j] = stream sample sbase + j
        self.apc_state = [torch.zeros(self.apc_eng.state_floats(), **f32) for _ in range(2)]
        self.lstm_state = [torch.zeros(self.a2f_pk["lstm"].state_floats(), **f32) for _ in range(2)]
        self.a2h_state = [torch.zeros(self.a2h_eng.state_bytes(), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.apc_i = self.lstm_i = self.a2h_i = 0                                # which buffer holds the current state
        self.a2h_started = False
        H = APC_model.hidden_size
        self.last = torch.zeros(1, H, **f32)                                     # the newest LLE row (odd row of a pair, and the tail)
        self.pend = torch.zeros(self.a2h_eng.max_audio_frames, 2 * H, **f32)         # pair rows not yet handed to the head-pose generator
        self.pend_row0 = self.pend_n = 0
        self._mel = self._feats = self._rows = self._x = None
        self._out_mouth: list = []
        self._out_pose: list = []

    # ---- the stages (run_plan calls them in order) ----------------------------------------------------------------------
    def feed(self, samples, first: int, keep_from: int) -> None:
        keep = keep_from - self.sbase                                           # samples before the next window are no longer read
        if keep > 0:
            self.sbuf[: self.slen - keep] = self.sbuf[keep: self.slen].clone()
            self.sbase += keep
            self.slen -= keep
        n = samples.shape[0]
        if self.slen + n > self.scap or first != self.sbase + self.slen:
            raise RuntimeError("internal: sample buffer overflow or gap")
        self.sbuf[self.slen: self.slen + n] = samples
        self.slen += n

    def mel(self, w0: int, w1: int, ended: bool) -> None:
        from . import mel as mel_mod
        off = window_start(w0) - self.sbase
        self._mel = mel_mod.compute_mel_range(self.sbuf[off: self.slen], self.sbase + off, w0, w1 - w0, ended, workspace=self.mel_ws)

    def apc(self, w0: int, w1: int) -> None:
        i = self.apc_i
        self._feats = self.apc_eng.forward_state(self._mel, self.apc_state[i] if w0 > 0 else None, self.apc_state[1 - i])
        self.apc_i = 1 - i

    def lle(self, w0: int, w1: int) -> None:
        from . import manifold
        f = self._feats
        if self.use_lle:
            f = manifold.project(f, self.db, self.knear, self.lle_percent)
        self._rows = self.torch.cat([self.last, f]) if w0 % 2 else f            # LLE rows from 2 * (w0 // 2) on
        self.last = f[-1:].clone()                                              # the odd row of the next pair; the tail at the end

    def pairs(self, p0: int, p1: int) -> None:
        x = self._rows[: 2 * (p1 - p0)].reshape(p1 - p0, -1)
        if self.pend_n + (p1 - p0) > self.pend.shape[0]:
            raise RuntimeError("internal: head-pose row buffer overflow")
        self.pend[self.pend_n: self.pend_n + (p1 - p0)] = x                    # waits there until the head-pose generator takes it
        self._x = (p0, self.pend[self.pend_n: self.pend_n + (p1 - p0)])
        self.pend_n += p1 - p0

    def mouth(self, steps, npairs: int, frames) -> None:
        torch = self.torch
        a0, a1 = steps
        parts = []
        if a0 < npairs:
            p0, x = self._x
            if p0 != a0 or p0 + x.shape[0] != npairs:
                raise RuntimeError("internal: Audio2Feature steps out of step with the pair rows")
            parts.append(x)
        if a1 > npairs:                                                         # the tail (finish): the last LLE row repeated
            parts.append(self.last.expand(2 * (a1 - max(a0, npairs)), -1).reshape(-1, 2 * self.last.shape[1]))
        x = torch.cat(parts) if len(parts) > 1 else parts[0].contiguous()
        pk = self.a2f_pk
        i = self.lstm_i
        h = pk["lstm"].forward_state(pk["d3"](pk["d0"](x)), self.lstm_state[i] if a0 > 0 else None, self.lstm_state[1 - i])
        self.lstm_i = 1 - i
        y = pk["f6"](pk["f3"](pk["f0"](h)))
        m0, m1 = frames
        if m1 > m0:
            self._out_mouth.append((m0, y[m0 + self.ff_mouth - a0:]))

    def poses(self, rows, frames) -> None:
        torch = self.torch
        (r0, r1), (h0, h1) = rows, frames
        if r0 != self.pend_row0 or r1 != self.pend_row0 + self.pend_n:
            raise RuntimeError("internal: head-pose rows out of step")
        nf = h1 - h0
        noise = expq = None
        if self.gmm:
            g = self.generator
            noise = torch.empty(nf, self.nd)
            expq = torch.empty(nf, self.nc)
            for k in range(nf):                 # draw_gmm_noise's order: the Exp(1) draws of multinomial, then randn, per frame
                expq[k] = torch.empty(1, self.nc).exponential_(1, generator=g)[0]
                noise[k] = torch.randn(1, self.nd, generator=g).float()[0]
            noise = noise.to(self.device)
            expq = expq.to(self.device) if self.nc > 1 else None
        i = self.a2h_i
        out = self.a2h_eng.generate_resume(self.pend[: self.pend_n] if self.pend_n else None, self.pend_row0, self.pre, noise, expq,
                                           self.sigma_scale, self.ff_head, h0, nf, self.a2h_state[i] if self.a2h_started else None,
                                           self.a2h_state[1 - i])
        self.a2h_i, self.a2h_started = 1 - i, True
        self.pend_row0 += self.pend_n
        self.pend_n = 0
        self._out_pose.append((h0, out))

    # ---- public --------------------------------------------------------------------------------------------------------
    def _run(self, plans, samples, host: bool) -> LiveFrames:
        torch = self.torch
        self._out_mouth, self._out_pose = [], []
        off = 0
        for plan in plans:
            n = plan.samples[1] - plan.samples[0]
            run_plan(self, plan, samples[off: off + n] if n else None)
            off += n
        # the status words, once per push (each read waits for the stream)
        for eng, what in ((self.apc_eng, "APC GRU"), (self.a2f_pk["lstm"], "Audio2Feature LSTM")):
            code = eng.status()
            if code != 0:
                raise RuntimeError("%s: inter-workgroup hand-off timed out (status 0x%x); the live session cannot continue" % (what, code))
        if self._out_pose:
            code = self.a2h_eng.status()
            if code != 0:
                raise RuntimeError("head-pose generator: status 0x%x (the carried state did not match its frame)" % code)
        mouth = torch.cat([t for _, t in self._out_mouth]) if self._out_mouth else torch.empty(0, self._mouth_dim(), device=self.device)
        poses = torch.cat([t for _, t in self._out_pose]) if self._out_pose else torch.empty(0, self.nd, device=self.device)
        m0 = self._out_mouth[0][0] if self._out_mouth else self.sched.m
        h0 = self._out_pose[0][0] if self._out_pose else self.sched.h
        self._mel = self._feats = self._rows = self._x = None
        if host:
            mouth, poses = mouth.cpu().numpy(), poses.cpu().numpy()
        return LiveFrames(mouth, m0, poses, h0)

    def _mouth_dim(self) -> int:
        return int(self.a2f_pk["f6"].out_features)

    def _samples(self, samples):
        torch = self.torch
        if isinstance(samples, torch.Tensor):
            if samples.dtype != torch.float32 or samples.dim() != 1:
                raise ValueError("samples must be a 1-d float32 array of 16 kHz audio (got %s %s)" % (samples.dtype, tuple(samples.shape)))
            return samples.to(self.device).contiguous()
        a = np.asarray(samples)
        if a.dtype != np.float32 or a.ndim != 1:
            raise ValueError("samples must be a 1-d float32 array of 16 kHz audio (got %s %s)" % (a.dtype, a.shape))
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def push(self, samples, host: bool = False) -> LiveFrames:
        """Take float32 16 kHz samples (host array or device tensor, any length); return the frames that became final."""
        if self.sched.ended:
            raise RuntimeError("the clip has ended (finish() was called): no more audio can be pushed")
        x = self._samples(samples)
        with self.torch.cuda.device(self.device):
            return self._run(self.sched.plan_push(x.shape[0]), x, host)

    def finish(self, host: bool = False) -> LiveFrames:
        """End of the clip: the zero-padded last windows, the Audio2Feature tail and the remaining head poses."""
        with self.torch.cuda.device(self.device):
            return self._run([self.sched.plan_finish()], None, host)
