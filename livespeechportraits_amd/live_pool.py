"""The device side of the live audio path, written once: ``LiveSessionPool`` advances 1..16 independent live sessions with ONE call per
stage and tick, whatever the number of open sessions (DESIGN.md "Live session pool").  ``live.LiveAudioFrontEnd`` is a pool of one.

The sessions share the models, the packed weights and the feature database; each has its own ``LiveScheduler`` (unchanged rules) and a
``PrimingPlanner`` that spreads the head-pose WaveNet's priming over the ticks.  ``run_pool_round`` merges the sessions' plans of one round
into one call per stage; the stages are the several-streams entry points (lspmel_compute_ranges, lsprnn_forward_multi,
lspa2h_generate_resume_multi) and the row-wise ones (KNN / LLE, the dense layers), whose rows do not depend on what shares the call.  So a
session's mouth rows and poses are bit for bit those of the whole-clip path whoever else is in the pool."""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from .live import MEL_WIN, LiveFrames, LiveScheduler, PrimingPlanner, window_start

MAX_SESSIONS = 16          # LSPRNN_MAX_SEQUENCES == LSPA2H_MAX_STREAMS == LSPMEL_MAX_SEGMENTS


def run_pool_round(backend, work) -> None:
    """One round of a tick.  ``work``: (key, LivePlan, samples, rows, steps) per session that has something to do, in ascending key order;
    rows / steps come from the session's PrimingPlanner.  Each stage of ``backend`` is called at most once, in this order, with the
    sessions that take part in it:
    feed [(key, samples, first_sample, keep_from)]   append the new samples; samples before `keep_from` are no longer read
    mel [(key, w0, w1, ended)]   apc / lle [(key, w0, w1)]   windows == rows [w0, w1)
    pairs [(key, p0, p1)]                     pair rows [p0, p1) from LLE rows [2 p0, 2 p1)
    mouth [(key, steps, npairs, frames)]      Audio2Feature steps [a0, a1) (>= npairs: the tail); emit mouth frames [m0, m1)
    poses [(key, rows, steps, frames)]        hand pair rows [r0, r1) to the head-pose generator, run its steps [s0, s1); emit poses [h0, h1)"""
    feed = [(k, smp, p.samples[0], window_start(p.windows[0])) for k, p, smp, _, _ in work if p.samples[1] > p.samples[0]]
    if feed:
        backend.feed(feed)
    win = [(k, p.windows[0], p.windows[1], p.ended) for k, p, _, _, _ in work if p.windows[1] > p.windows[0]]
    if win:
        backend.mel(win)
        backend.apc([w[:3] for w in win])
        backend.lle([w[:3] for w in win])
    pairs = [(k, p.pairs[0], p.pairs[1]) for k, p, _, _, _ in work if p.pairs[1] > p.pairs[0]]
    if pairs:
        backend.pairs(pairs)
    mouth = [(k, p.a2f_steps, p.pairs[1], p.mouth) for k, p, _, _, _ in work if p.a2f_steps[1] > p.a2f_steps[0]]
    if mouth:
        backend.mouth(mouth)
    poses = [(k, rows, steps, p.poses) for k, p, _, rows, steps in work if steps[1] > steps[0]]
    if poses:
        backend.poses(poses)


class PoolPlanner:
    """The host side of a pool, without a device: session ids, slots, one LiveScheduler and one PrimingPlanner per session, and the merge of
    a tick into rounds.  LiveSessionPool drives the device with it; tests/test_live_pool_cpu.py drives a provenance fake."""

    def __init__(self, max_sessions: int, ff_mouth: int, ff_head: int, field: int, max_chunk_samples: int, prime_steps_per_tick: int):
        if not 1 <= max_sessions <= MAX_SESSIONS:
            raise ValueError("max_sessions must be in 1..%d" % MAX_SESSIONS)
        if max_chunk_samples < 1:
            raise ValueError("max_chunk_samples must be >= 1")
        self.max_sessions = max_sessions
        self.args = (ff_mouth, ff_head, max_chunk_samples)
        self.field, self.per_tick = field, prime_steps_per_tick
        PrimingPlanner(field, ff_head, prime_steps_per_tick)                   # validates
        self.free = list(range(max_sessions))
        self.slot: Dict[int, int] = {}                                        # open session id -> slot
        self.sched: Dict[int, LiveScheduler] = {}
        self.prime: Dict[int, PrimingPlanner] = {}
        self.next_id = 0

    def open(self) -> int:
        if not self.free:
            raise RuntimeError("all %d sessions of the pool are open: close one first (max_sessions)" % self.max_sessions)
        sid, self.next_id = self.next_id, self.next_id + 1
        self.slot[sid] = self.free.pop(0)
        self.sched[sid] = LiveScheduler(*self.args)
        self.prime[sid] = PrimingPlanner(self.field, self.args[1], self.per_tick)
        return sid

    def close(self, sid: int) -> None:
        self.check(sid)
        self.free.append(self.slot.pop(sid))
        self.free.sort()
        del self.sched[sid], self.prime[sid]

    def check(self, sid) -> None:
        if sid not in self.slot:
            if isinstance(sid, int) and 0 <= sid < self.next_id:
                raise RuntimeError("session %d is closed (finish() or close() was called): no more audio can be pushed" % sid)
            raise KeyError("unknown session id %r" % (sid,))

    def rounds(self, lengths: Dict[int, int], finish) -> List[list]:
        """Plans of one tick: ``lengths`` = samples pushed per session, ``finish`` = sessions that end after them.  -> per round the list of
        (sid, LivePlan, (offset, n) into the session's samples, rows, steps) in ascending session id."""
        per: Dict[int, list] = {}
        for sid in sorted(set(lengths) | set(finish)):
            self.prime[sid].begin_tick()
            plans = self.sched[sid].plan_push(lengths.get(sid, 0))
            if sid in finish:
                plans.append(self.sched[sid].plan_finish())
            off, items = 0, []
            for p in plans:
                n = p.samples[1] - p.samples[0]
                rows, steps = self.prime[sid].plan(p.pairs[1], p.poses)
                items.append((sid, p, (off, n), rows, steps))
                off += n
            per[sid] = items
        nrounds = max([len(v) for v in per.values()], default=0)
        return [[per[sid][r] for sid in sorted(per) if r < len(per[sid])] for r in range(nrounds)]


    def preview(self, lengths: Dict[int, int], finish) -> Dict[int, tuple]:
        """What ``rounds(lengths, finish)`` would hand out, without advancing anything: {sid: (mouth rows, head poses)} that the tick makes
        final.  Runs ``rounds`` on deep copies of the named sessions' schedulers."""
        import copy
        named = sorted(set(lengths) | set(finish))
        twin = copy.copy(self)
        twin.sched = {sid: copy.deepcopy(self.sched[sid]) for sid in named}
        twin.prime = {sid: copy.deepcopy(self.prime[sid]) for sid in named}
        out = {sid: [0, 0] for sid in named}
        for work in twin.rounds(lengths, finish):
            for sid, p, _, _, _ in work:
                out[sid][0] += p.mouth[1] - p.mouth[0]
                out[sid][1] += p.poses[1] - p.poses[0]
        return {sid: tuple(v) for sid, v in out.items()}


class _Slot:
    """Host-side book-keeping of one open session (the device memory is the pool's slot arrays)."""

    def __init__(self, slot: int, pre, generator):
        self.slot, self.pre, self.generator = slot, pre, generator
        self.sbase = self.slen = 0                    # the slot's sample buffer holds stream samples [sbase, sbase + slen)
        self.apc_i = self.lstm_i = self.a2h_i = 0     # which of the two state buffers holds the current state
        self.pend_row0 = self.pend_n = 0              # pair rows not yet handed to the head-pose generator
        self.out_mouth: list = []
        self.out_pose: list = []


class LiveSessionPool:
    """Up to ``max_sessions`` (<= 16) live streams on one device, advanced together.

    Built from what demo.py:146-166 builds and reads from the config (see LiveAudioFrontEnd, the pool of one); the per-session
    ``pre_headpose`` / ``generator`` are arguments of ``open``.  ``tick``
    pushes samples to any subset of the open sessions and returns each one's LiveFrames; per stage it makes one call, so the number of
    launches per tick does not depend on the number of sessions.  A session's outputs are bit for bit those of the
    whole-clip path on its own audio, whoever else is in the pool.  The head-pose WaveNet's priming (field - 1 steps before pose 0) runs
    ``prime_steps_per_tick`` steps per tick from the first pair row on, so a session that joins does not stall the others' tick.
    GMM noise: per session, per head-pose frame, in frame order, from the session's ``generator`` in draw_gmm_noise's order; sessions
    opened with ``generator=None`` share the global generator, and the draws of a round go in ascending session id -- so with the global
    generator a session's poses depend on who else draws; give every session its own generator for poses that do not.
    Device memory is fixed at construction.  The status words are read once per round (a tick is one round unless a push is longer
    than ``max_chunk_samples``); a lost inter-workgroup hand-off (another stream holding the CUs for the whole time-out) ends the pool
    with an error.  Every stage keeps its input state in a buffer of its own (two per stage and slot, used in turn), so a caller that
    drives the C entry points directly can run a failed call again from the same state."""

    def __init__(self, APC_model, Audio2Feature, Audio2Headpose, APC_feat_database, use_LLE: bool, Knear: int, LLE_percent: float,
                 sigma_scale: float = 0.3, device="cuda:0", max_sessions: int = 16, max_chunk_samples: int = 16000, feature_opt=None,
                 headpose_opt=None, prime_steps_per_tick: int = 16):
        import torch
        self.torch = torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("LiveSessionPool runs on the MI355X only: device must be a GPU (there is no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if getattr(APC_model, "rnn_residual", False):
            raise NotImplementedError("residual APC stacks are not supported (no shipped config enables them)")
        fo = feature_opt if feature_opt is not None else Audio2Feature.opt
        ho = headpose_opt if headpose_opt is not None else Audio2Headpose.opt
        if getattr(ho, "feature_decoder", "WaveNet") != "WaveNet":
            raise NotImplementedError("the live path generates head poses with the WaveNet decoder only (the LSTM decoder is in no shipped config)")
        if not 1 <= max_sessions <= MAX_SESSIONS:
            raise ValueError("max_sessions must be in 1..%d" % MAX_SESSIONS)
        if max_chunk_samples < 1:
            raise ValueError("max_chunk_samples must be >= 1")
        self.device = dev
        S = self.max_sessions = int(max_sessions)
        self.ff_mouth, self.ff_head = int(fo.frame_future), int(ho.frame_future)
        self.use_lle, self.knear, self.lle_percent = bool(use_LLE), int(Knear), float(LLE_percent)
        self.sigma_scale = float(sigma_scale)
        self.nd, self.nc, self.gmm = int(ho.A2H_GMM_ndim), int(ho.A2H_GMM_ncenter), ho.loss == "GMM"
        f32 = dict(dtype=torch.float32, device=dev)
        max_win = 2 * (max_chunk_samples // MEL_WIN + 2) + 2                   # windows that one step can make final
        max_pairs = max_win // 2 + 1
        self.apc_eng = APC_model._get_engine(dev, S * max_win)
        a2f = Audio2Feature.Audio2Feature
        a2f = a2f.module if hasattr(a2f, "module") else a2f
        self.a2f_pk = a2f._pack(dev, S * (max_pairs + self.ff_mouth))
        net = Audio2Headpose._net()
        # a head-pose engine of its own: its workspace holds the sessions' projection rings (whole-clip calls would overwrite a shared one)
        from .a2h_engine import HeadposeEngine
        o = net.opt
        ring = max_pairs + self.ff_head + 1                                    # >= PrimingPlanner.ring_rows_needed(ff_head, max_pairs)
        assert ring >= PrimingPlanner.ring_rows_needed(self.ff_head, max_pairs)
        self.a2h_eng = HeadposeEngine(o.A2H_wavenet_residual_layers, o.A2H_wavenet_residual_blocks, o.A2H_wavenet_residual_channels,
                                      o.A2H_wavenet_dilation_channels, o.A2H_wavenet_skip_channels, o.A2H_wavenet_kernel_size,
                                      o.A2H_wavenet_input_channels, o.A2H_wavenet_cond_channels, o.APC_hidden_size,
                                      o.A2H_GMM_ncenter, o.A2H_GMM_ndim, o.loss, max_audio_frames=ring)
        self.a2h_eng.load_state_dict({k: v for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")})
        self.a2h_eng.bind(dev)
        self.a2h_eng.bind_multi(S)
        self.plan = PoolPlanner(S, self.ff_mouth, self.ff_head, int(self.a2h_eng.receptive_field), max_chunk_samples, prime_steps_per_tick)
        self.db = torch.as_tensor(np.ascontiguousarray(APC_feat_database, np.float32)).to(dev) if self.use_lle else None
        from . import _native as N
        lib = N.load()
        self.mel_ws = torch.empty(int(lib.lspmel_workspace_bytes(S * max_win)), dtype=torch.uint8, device=dev)
        # the slot arrays
        self.scap = max_chunk_samples + 4 * MEL_WIN
        self.sbuf = torch.zeros(S * self.scap, **f32)
        self.apc_state = torch.zeros(2, S, self.apc_eng.state_floats(), **f32)
        self.lstm_state = torch.zeros(2, S, self.a2f_pk["lstm"].state_floats(), **f32)
        self.a2h_state = torch.zeros(2, S, self.a2h_eng.state_bytes(), dtype=torch.uint8, device=dev)
        self.H = H = APC_model.hidden_size
        self.last = torch.zeros(S, H, **f32)                                    # the newest LLE row of each session
        self.ring = ring
        self.pend = torch.zeros(S * ring, 2 * H, **f32)                         # pair rows not yet handed to the head-pose generator
        self.sess: Dict[int, _Slot] = {}
        self._round_reset()

    # ---- sessions ----------------------------------------------------------------------------------------------------------------
    def open(self, pre_headpose, generator=None) -> int:
        """A new session in a free slot -> its id (never reused; the slot is).  Starts from zeros: the first call of every stage takes no
        carried state, and the slot's newest-LLE-row is cleared."""
        torch = self.torch
        pre = torch.as_tensor(np.ascontiguousarray(np.asarray(pre_headpose, np.float32).reshape(-1))).to(self.device)
        sid = self.plan.open()
        slot = self.plan.slot[sid]
        self.sess[sid] = _Slot(slot, pre, generator)
        with torch.cuda.device(self.device):
            self.last[slot].zero_()
        return sid

    def close(self, sid: int) -> None:
        self.plan.close(sid)
        del self.sess[sid]

    @property
    def open_sessions(self) -> List[int]:
        return sorted(self.sess)

    # ---- the stages (run_pool_round calls each at most once per round) -----------------------------------------------------------
    def _round_reset(self) -> None:
        self._mel = self._feats = self._src = self._seq = self._X = self._xat = None
        self._ran_poses = False

    def _joined(self, parts):
        """torch.cat(parts) -- without a launch when the parts already lie one after another in one buffer (the usual case: slices of one
        upload, or of one stage's output), so that the launches of a tick do not depend on the number of sessions."""
        torch = self.torch
        if len(parts) == 1:
            return parts[0]
        t0 = parts[0]
        row = t0.stride(0) if t0.dim() else 1
        end = t0.data_ptr()
        for t in parts:
            if t.data_ptr() != end or not t.is_contiguous() or t.shape[1:] != t0.shape[1:] or t.untyped_storage().data_ptr() != t0.untyped_storage().data_ptr():
                return torch.cat(parts)
            end += t.numel() * t.element_size()
        n = sum(t.shape[0] for t in parts)
        return torch.as_strided(t0, (n,) + tuple(t0.shape[1:]), t0.stride(), t0.storage_offset())

    def _index(self, values) -> "object":
        return self.torch.from_numpy(np.asarray(values, np.int64)).to(self.device, non_blocking=True)

    def feed(self, items) -> None:
        src_keep, dst_keep, dst_new, new = [], [], [], []
        for sid, samples, first, keep_from in items:
            s = self.sess[sid]
            base = s.slot * self.scap
            keep = keep_from - s.sbase                                         # samples before the next window are no longer read
            if keep > 0:
                n = s.slen - keep
                src_keep.append(np.arange(base + keep, base + s.slen))
                dst_keep.append(np.arange(base, base + n))
                s.sbase += keep
                s.slen = n
            n = samples.shape[0]
            if s.slen + n > self.scap or first != s.sbase + s.slen:
                raise RuntimeError("internal: sample buffer overflow or gap")
            dst_new.append(np.arange(base + s.slen, base + s.slen + n))
            new.append(samples)
            s.slen += n
        if src_keep:
            nk = sum(len(a) for a in src_keep)
            idx = self._index(np.concatenate(src_keep + dst_keep))
            self.sbuf.index_copy_(0, idx[nk:], self.sbuf.index_select(0, idx[:nk]))
        self.sbuf.index_copy_(0, self._index(np.concatenate(dst_new)), self._joined(new))

    def mel(self, items) -> None:
        from . import mel as mel_mod
        segs = []
        for sid, w0, w1, ended in items:
            s = self.sess[sid]
            off = window_start(w0) - s.sbase
            base = s.slot * self.scap
            segs.append((self.sbuf[base + off: base + s.slen], s.sbase + off, w0, w1 - w0, ended))
        self._mel = mel_mod.compute_mel_ranges(segs, workspace=self.mel_ws)

    def apc(self, items) -> None:
        sin, sout = [], []
        for sid, w0, w1 in items:
            s = self.sess[sid]
            sin.append(self.apc_state[s.apc_i, s.slot] if w0 > 0 else None)
            sout.append(self.apc_state[1 - s.apc_i, s.slot])
            s.apc_i = 1 - s.apc_i
        self._feats = self.apc_eng.forward_multi(self._mel, [w1 - w0 for _, w0, w1 in items], sin, sout)

    def lle(self, items) -> None:
        from . import manifold
        torch = self.torch
        f = self._feats
        if self.use_lle:
            f = manifold.project(f, self.db, self.knear, self.lle_percent)
        S = self.max_sessions
        self._src = torch.cat([self.last, f])                                   # rows 0..S-1: each slot's newest LLE row BEFORE this round
        self._seq = {}
        off, slots, lasts = S, [], []
        for sid, w0, w1 in items:
            s = self.sess[sid]
            seq = list(range(off, off + w1 - w0))
            self._seq[sid] = ([s.slot] + seq) if w0 % 2 else seq                # LLE rows from 2 * (w0 // 2) on
            off += w1 - w0
            slots.append(s.slot)
            lasts.append(off - 1)
        idx = self._index(slots + lasts)
        self.last.index_copy_(0, idx[:len(slots)], self._src.index_select(0, idx[len(slots):]))   # the odd row of the next pair; the tail

    def pairs(self, items) -> None:
        src_idx, dst_idx = [], []
        self._xat = {}
        at = 0
        for sid, p0, p1 in items:
            s = self.sess[sid]
            n = p1 - p0
            if s.pend_n + n > self.ring:
                raise RuntimeError("internal: head-pose row buffer overflow")
            src_idx += self._seq[sid][: 2 * n]
            dst_idx += range(s.slot * self.ring + s.pend_n, s.slot * self.ring + s.pend_n + n)
            self._xat[sid] = (p0, at, n)
            at += n
            s.pend_n += n
        idx = self._index(src_idx + dst_idx)
        self._X = self._src.index_select(0, idx[:len(src_idx)]).view(at, 2 * self.H)
        self.pend.index_copy_(0, idx[len(src_idx):], self._X)                   # waits there until the head-pose generator takes it

    def mouth(self, items) -> None:
        torch = self.torch
        nx = self._X.shape[0] if self._X is not None else 0
        tail = torch.cat([self.last, self.last], 1)                             # the tail (finish): the last LLE row repeated
        src = torch.cat([self._X, tail]) if nx else tail
        idx, lengths, sin, sout = [], [], [], []
        for sid, (a0, a1), npairs, _ in items:
            s = self.sess[sid]
            if a0 < npairs:
                p0, at, n = self._xat[sid] if self._xat and sid in self._xat else (None, 0, 0)
                if p0 != a0 or p0 + n != npairs:
                    raise RuntimeError("internal: Audio2Feature steps out of step with the pair rows")
                idx += range(at, at + n)
            if a1 > npairs:
                idx += [nx + s.slot] * (a1 - max(a0, npairs))
            lengths.append(a1 - a0)
            sin.append(self.lstm_state[s.lstm_i, s.slot] if a0 > 0 else None)
            sout.append(self.lstm_state[1 - s.lstm_i, s.slot])
            s.lstm_i = 1 - s.lstm_i
        pk = self.a2f_pk
        x = src.index_select(0, self._index(idx))
        h = pk["lstm"].forward_multi(pk["d3"](pk["d0"](x)), lengths, sin, sout)
        y = pk["f6"](pk["f3"](pk["f0"](h)))
        off, rows, emit = 0, [], []
        for (sid, (a0, a1), _, (m0, m1)), n in zip(items, lengths):
            if m1 > m0:
                emit.append((sid, m0, len(rows), n - (m0 + self.ff_mouth - a0)))
                rows += range(off + m0 + self.ff_mouth - a0, off + n)
            off += n
        if rows:                                                                # the emitted rows of all sessions, one after another
            ysel = y.index_select(0, self._index(rows))
            for sid, m0, at, n in emit:
                self.sess[sid].out_mouth.append((m0, ysel[at: at + n]))

    def poses(self, items) -> None:
        torch = self.torch
        f1 = self.a2h_eng.receptive_field - 1
        rows_idx, frames = [], []
        for sid, (r0, r1), (s0, s1), (h0, h1) in items:
            s = self.sess[sid]
            if r0 != s.pend_row0 or r1 != s.pend_row0 + s.pend_n or max(s1 - f1, 0) != h1 or (h1 > h0 and max(s0 - f1, 0) != h0):
                raise RuntimeError("internal: head-pose rows or steps out of step")
            rows_idx += range(s.slot * self.ring, s.slot * self.ring + s.pend_n)
            frames.append(h1 - h0)
        nf = sum(frames)
        noise = expq = None
        if self.gmm and nf:
            noise = torch.empty(nf, self.nd)
            expq = torch.empty(nf, self.nc)
            k = 0
            for (sid, _, _, _), n in zip(items, frames):      # ascending session id; per frame draw_gmm_noise's order: Exp(1) draws, then randn
                g = self.sess[sid].generator
                for _ in range(n):
                    expq[k] = torch.empty(1, self.nc).exponential_(1, generator=g)[0]
                    noise[k] = torch.randn(1, self.nd, generator=g).float()[0]
                    k += 1
            noise = noise.to(self.device)
            expq = expq.to(self.device) if self.nc > 1 else None
        out = torch.empty(nf, self.nd, dtype=torch.float32, device=self.device)
        audio = self.pend.index_select(0, self._index(rows_idx)) if rows_idx else None
        streams, k = [], 0
        for (sid, _, (s0, s1), (h0, h1)), n in zip(items, frames):
            s = self.sess[sid]
            streams.append(dict(slot=s.slot, row0=s.pend_row0, n_new=s.pend_n, step0=s0, step1=s1, pre=s.pre,
                                noise=noise[k:k + n] if noise is not None and n else None, expq=expq[k:k + n] if expq is not None and n else None,
                                state_in=self.a2h_state[s.a2h_i, s.slot] if s0 > 0 else None, state_out=self.a2h_state[1 - s.a2h_i, s.slot],
                                out=out[k:k + n]))
            s.a2h_i = 1 - s.a2h_i
            s.pend_row0 += s.pend_n
            s.pend_n = 0
            if n:
                s.out_pose.append((h0, out[k:k + n]))
            k += n
        self.a2h_eng.generate_resume_multi(streams, audio, self.sigma_scale, self.ff_head)
        self._ran_poses = True

    # ---- public ------------------------------------------------------------------------------------------------------------------
    def _samples(self, sid, samples):
        torch = self.torch
        if isinstance(samples, torch.Tensor):
            if samples.dtype != torch.float32 or samples.dim() != 1:
                raise ValueError("session %d: samples must be a 1-d float32 array of 16 kHz audio (got %s %s)" % (sid, samples.dtype, tuple(samples.shape)))
            return samples
        a = np.asarray(samples)
        if a.dtype != np.float32 or a.ndim != 1:
            raise ValueError("session %d: samples must be a 1-d float32 array of 16 kHz audio (got %s %s)" % (sid, a.dtype, a.shape))
        return a

    def _status(self) -> None:
        for eng, what in ((self.apc_eng, "APC GRU"), (self.a2f_pk["lstm"], "Audio2Feature LSTM")):
            code = eng.status()
            if code != 0:
                raise RuntimeError("%s: inter-workgroup hand-off timed out (status 0x%x); the pool cannot continue" % (what, code))
        if self._ran_poses:
            code = self.a2h_eng.status_multi()
            if code != 0:
                raise RuntimeError("head-pose generator: status 0x%x (a carried state did not match its step)" % code)

    def tick(self, samples=None, finish=(), host: bool = False) -> Dict[int, LiveFrames]:
        """Push ``samples`` ({session id: float32 16 kHz samples, host array or device tensor, any length}, or (id, samples) pairs) and end
        the sessions in ``finish`` (after their samples, if any; they are closed afterwards).  -> {id: LiveFrames} of the frames that
        became final, for every session named.  Nothing is changed when an argument is refused."""
        torch = self.torch
        pairs = list(samples.items()) if hasattr(samples, "items") else list(samples or ())
        finish = list(finish)
        given: Dict[int, object] = {}
        for sid, smp in pairs:
            if sid in given:
                raise ValueError("session %d appears twice in one tick" % sid)
            self.plan.check(sid)
            given[sid] = self._samples(sid, smp)
        if len(set(finish)) != len(finish):
            raise ValueError("a session appears twice in finish")
        for sid in finish:
            self.plan.check(sid)
        # one upload for all host arrays; device tensors are taken as they are
        host_ids = [sid for sid in sorted(given) if isinstance(given[sid], np.ndarray) and given[sid].shape[0]]
        with torch.cuda.device(self.device):
            if host_ids:
                flat = torch.from_numpy(np.ascontiguousarray(np.concatenate([given[sid] for sid in host_ids]))).to(self.device)
                off = 0
                for sid in host_ids:
                    n = given[sid].shape[0]
                    given[sid] = flat[off: off + n]
                    off += n
            for sid in given:
                if isinstance(given[sid], np.ndarray):
                    given[sid] = torch.empty(0, dtype=torch.float32, device=self.device)
                else:
                    given[sid] = given[sid].to(self.device).contiguous()
            named = sorted(set(given) | set(finish))
            for sid in named:
                self.sess[sid].out_mouth, self.sess[sid].out_pose = [], []
            for work in self.plan.rounds({sid: int(t.shape[0]) for sid, t in given.items()}, set(finish)):
                self._round_reset()
                run_pool_round(self, [(sid, p, given[sid][o: o + n] if n else None, rows, steps) for sid, p, (o, n), rows, steps in work])
                self._status()
            self._round_reset()
            result = self._collect(named, host)
        for sid in finish:
            self.close(sid)
        return result

    def _collect(self, named, host: bool) -> Dict[int, LiveFrames]:
        torch = self.torch
        mdim = int(self.a2f_pk["f6"].out_features)
        parts = {"m": [], "p": []}
        spans = {}
        for sid in named:
            s = self.sess[sid]
            sched = self.plan.sched[sid]
            m0 = s.out_mouth[0][0] if s.out_mouth else sched.m
            h0 = s.out_pose[0][0] if s.out_pose else sched.h
            nm, nh = sum(t.shape[0] for _, t in s.out_mouth), sum(t.shape[0] for _, t in s.out_pose)
            parts["m"] += [t for _, t in s.out_mouth]
            parts["p"] += [t for _, t in s.out_pose]
            spans[sid] = (m0, nm, h0, nh)
            s.out_mouth, s.out_pose = [], []
        mouth = self._joined(parts["m"]) if parts["m"] else torch.empty(0, mdim, device=self.device)
        poses = self._joined(parts["p"]) if parts["p"] else torch.empty(0, self.nd, device=self.device)
        if host:                                                                # one copy per kind, whatever the number of sessions
            mouth, poses = mouth.cpu().numpy(), poses.cpu().numpy()
        out, am, ap = {}, 0, 0
        for sid in named:
            m0, nm, h0, nh = spans[sid]
            out[sid] = LiveFrames(mouth[am: am + nm], m0, poses[ap: ap + nh], h0)
            am, ap = am + nm, ap + nh
        return out
