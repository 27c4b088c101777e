"""GPU tests of the several-streams entry points (lsprnn_forward_multi, lspa2h_generate_resume_multi, lspmel_compute_ranges) and of the
LiveSessionPool on top of them.  The acceptance test is "S streams in one call == each stream alone, bit for bit": the stream alone is
pinned on the whole-clip path by tests/test_gpu_live.py and that on the reference goldens.  No tolerance of its own."""
import time

import numpy as np
import pytest
import torch

from test_a2h_cpu import load_case
from test_gpu_live import (A2H_TOL, CLIP_FRAMES, CLIP_SAMPLES, DEV, RNN_CASES, _a2h_engine, _checked, _resume_chain, _rnn, frame_pieces,
                           models, session, wave_of, whole_clip)  # noqa: F401  (models: the module-scoped fixture)

pytestmark = pytest.mark.gpu


# ---- recurrent stacks: several sequences per launch ----------------------------------------------------------------------
RAGGED = {1: [37], 3: [1, 0, 60], 16: [0, 1, 5, 40, 17, 3, 64, 2, 33, 1, 90, 8, 21, 50, 13, 29]}      # sums <= 512 (max_steps of _rnn)


def _rand_states(e, n, rng):
    return [torch.from_numpy((rng.standard_normal(e.state_floats()) * 0.5).astype(np.float32)).to(DEV) for _ in range(n)]


@pytest.mark.parametrize("S", [1, 3, 16])
@pytest.mark.parametrize("route", ["wave", "layers"])
@pytest.mark.parametrize("case", sorted(RNN_CASES))
def test_forward_multi_equals_each_sequence_alone(case, route, S):
    e, _ = _rnn(case, route)
    lengths = RAGGED[S]
    rng = np.random.default_rng(100 + S)
    x = torch.from_numpy(rng.standard_normal((sum(lengths), e.input_size)).astype(np.float32) * 0.5).to(DEV)
    sin = _rand_states(e, S, rng)
    if S > 1:
        sin[-1] = None                                                     # one sequence starts from zeros
    offs = np.concatenate([[0], np.cumsum(lengths)])
    # each sequence alone
    alone, alone_state = [], []
    for s, T in enumerate(lengths):
        so = torch.full((e.state_floats(),), 7.0, device=DEV)
        if T:
            alone.append(_checked(e, lambda: e.forward_state(x[offs[s]:offs[s + 1]].contiguous(), sin[s], so)).cpu())
        else:
            alone.append(torch.empty(0, e.hidden_size))
        alone_state.append(so.cpu())
    # one call
    souts = [torch.full((e.state_floats(),), 7.0, device=DEV) for _ in range(S)]
    got = _checked(e, lambda: e.forward_multi(x, lengths, sin, souts)).cpu()
    for s, T in enumerate(lengths):
        assert torch.equal(got[offs[s]:offs[s + 1]], alone[s]), "sequence %d (T = %d)" % (s, T)
        assert torch.equal(souts[s].cpu(), alone_state[s]), "final state of sequence %d (T = %d)" % (s, T)
        if T == 0:
            assert bool((souts[s] == 7.0).all()), "the state-out slot of an empty sequence was written"
    # two chained calls with another grouping of the same sequences: first parts in order, second parts in reverse order
    cut = [T // 2 for T in lengths]
    mid = [torch.full((e.state_floats(),), 7.0, device=DEV) for _ in range(S)]
    xa = torch.cat([x[offs[s]:offs[s] + cut[s]] for s in range(S)]) if sum(cut) else None
    parts_a = _checked(e, lambda: e.forward_multi(xa, cut, sin, mid)).cpu() if xa is not None else torch.empty(0, e.hidden_size)
    order = [s for s in reversed(range(S)) if lengths[s] - cut[s] > 0]
    xb = torch.cat([x[offs[s] + cut[s]:offs[s + 1]] for s in order])
    fin = {s: torch.full((e.state_floats(),), 7.0, device=DEV) for s in order}
    parts_b = _checked(e, lambda: e.forward_multi(xb, [lengths[s] - cut[s] for s in order],
                                                  [mid[s] if cut[s] else sin[s] for s in order], [fin[s] for s in order])).cpu()
    oa = np.concatenate([[0], np.cumsum(cut)])
    ob = np.concatenate([[0], np.cumsum([lengths[s] - cut[s] for s in order])])
    for i, s in enumerate(order):
        whole = torch.cat([parts_a[oa[s]:oa[s + 1]], parts_b[ob[i]:ob[i + 1]]])
        assert torch.equal(whole, alone[s]), "chained, sequence %d" % s
        assert torch.equal(fin[s].cpu(), alone_state[s]), "chained final state, sequence %d" % s


@pytest.mark.parametrize("route", ["wave", "layers"])
def test_forward_multi_refusals(route):
    from livespeechportraits_amd import _native as N
    e, _ = _rnn("a2f_lstm", route)
    x = torch.zeros(8, e.input_size, device=DEV)
    a, b = (torch.zeros(e.state_floats(), device=DEV) for _ in range(2))
    with pytest.raises(N.LsprnnError, match="separate"):
        e.forward_multi(x, [4, 4], [a, None], [b, a])                      # a is sequence 0's input and sequence 1's output
    with pytest.raises(N.LsprnnError, match="separate"):
        e.forward_multi(x, [4, 4], [a, b], [a, None])
    with pytest.raises(N.LsprnnError, match="share"):
        e.forward_multi(x, [4, 4], None, [a, a])
    big = torch.zeros(e.max_steps + 1, e.input_size, device=DEV)
    with pytest.raises(N.LsprnnError, match="max_steps"):
        e.forward_multi(big, [e.max_steps, 1])
    with pytest.raises(ValueError):
        e.forward_multi(x, [4, 3])
    with pytest.raises(ValueError):
        e.forward_multi(x, [1] * 17)
    # nothing to do: no launch, nothing touched
    s = torch.full((e.state_floats(),), 7.0, device=DEV)
    assert e.forward_multi(torch.zeros(0, e.input_size, device=DEV), [0, 0], None, [s, None]).shape[0] == 0
    assert bool((s == 7.0).all())


# ---- head poses: several streams per launch, priming in slices -----------------------------------------------------------
def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _bounds(total, F1, prime_slice, frame_cuts):
    """Step boundaries of one stream: priming in slices of `prime_slice` steps (capped at the steps left), then frames cut at frame_cuts."""
    b, s = [0], 0
    while s < F1:
        s = min(F1, s + prime_slice)
        b.append(s)
    for f in frame_cuts:
        if F1 + f > b[-1] and F1 + f < total:
            b.append(F1 + f)
    if b[-1] != total:
        b.append(total)
    return b


def _run_streams(e, cfg, specs, sigma, ff, pass_all_rows=False):
    """specs: per stream dict(audio, pre, noise, expq, bounds, slot).  Runs rounds: in round r every stream that still has a step range
    takes part with its r-th range, passing the audio rows the range needs that it has not passed.  -> per-stream poses."""
    gmm = cfg["loss"] == "GMM"
    F1 = e.receptive_field - 1
    st = [dict(rows=0, state=None, bufs=[torch.empty(e.state_bytes(), dtype=torch.uint8, device=DEV) for _ in range(2)], i=0, outs=[])
          for _ in specs]
    rounds = max(len(sp["bounds"]) - 1 for sp in specs)
    for r in range(rounds):
        calls, rows = [], []
        for k, sp in enumerate(specs):
            if r + 1 >= len(sp["bounds"]):
                continue
            s0, s1 = sp["bounds"][r], sp["bounds"][r + 1]
            need = max(0, s1 - 1 + ff - F1) + 1
            if pass_all_rows:
                need = sp["audio"].shape[0]
            f0, f1 = max(s0 - F1, 0), max(s1 - F1, 0)
            new = sp["audio"][st[k]["rows"]:need] if need > st[k]["rows"] else sp["audio"][:0]
            so = st[k]["bufs"][st[k]["i"]]
            calls.append((k, dict(slot=sp["slot"], row0=st[k]["rows"], n_new=new.shape[0], step0=s0, step1=s1, pre=_d(sp["pre"]),
                                  noise=_d(sp["noise"][f0:f1]) if gmm and f1 > f0 else None,
                                  expq=_d(sp["expq"][f0:f1]) if gmm and cfg["ncenter"] > 1 and f1 > f0 else None,
                                  state_in=st[k]["state"], state_out=so)))
            rows.append(new)
            st[k]["rows"] = max(st[k]["rows"], need)
            st[k]["state"], st[k]["i"] = so, 1 - st[k]["i"]
        allrows = np.concatenate(rows) if rows else None
        outs = e.generate_resume_multi([c for _, c in calls], _d(allrows) if allrows is not None and len(allrows) else None, sigma, ff)
        assert e.status_multi() == 0
        for (k, _), o in zip(calls, outs):
            st[k]["outs"].append(o.cpu().numpy())
    return [np.concatenate(s["outs"]) for s in st]


@pytest.mark.parametrize("S", [1, 4, 16])
@pytest.mark.parametrize("name", ["default_n300", "nc2_l4b1"])
def test_generate_resume_multi_equals_each_stream_alone(name, S):
    from test_gpu_a2h import make_engine, run
    meta, cfg, sd, audio, pre, ref, noise, expq = load_case(name)
    sigma, ff = meta["sigma_scale"], meta["frame_future"]
    dev = torch.device(DEV)
    whole_eng = make_engine(cfg, sd, dev)
    e = _a2h_engine(cfg, sd, audio.shape[0])
    e.bind_multi(S)
    F1 = e.receptive_field - 1
    n = audio.shape[0] - ff
    slices = [1, 16, 100, F1]                                              # priming in slices of 1, 16, 100 steps, and in one go
    specs, wholes = [], []
    for k in range(S):
        off = (k * 3) % max(n - 2, 1)                                       # the same clip at different offsets
        a = audio[off:]
        nf = a.shape[0] - ff
        cuts = sorted({1 + k, nf // 2, nf - 1 - (k % 3)})
        specs.append(dict(audio=a, pre=pre, noise=noise[:nf], expq=expq[:nf] if expq is not None else None, slot=(S - 1 - k),
                          bounds=_bounds(F1 + nf, F1, slices[k % 4], [c for c in cuts if 0 < c < nf])))
        wholes.append(run(whole_eng, cfg, a, pre, noise[:nf], expq[:nf] if expq is not None else None, sigma, ff, dev))
    got = _run_streams(e, cfg, specs, sigma, ff)
    for k in range(S):
        assert np.array_equal(got[k], wholes[k]), "stream %d (priming slices of %d)" % (k, slices[k % 4])
    assert np.abs(got[0] - ref).max() <= A2H_TOL                            # stream 0 is the clip of the golden (offset 0)
    # ... and the chain of single-stream calls
    assert np.array_equal(got[0], _resume_chain(e, cfg, audio, pre, noise, expq, sigma, ff, [n // 2]))


def test_generate_resume_multi_ring_wrap():
    """One step per call through rings of frame_future + 2 rows: the rows wrap around every stream's ring many times, so the copy kernel's
    row table is exercised at every position."""
    from test_gpu_a2h import make_engine, run
    meta, cfg, sd, audio, pre, ref, noise, expq = load_case("nc2_l4b1")
    sigma, ff = meta["sigma_scale"], meta["frame_future"]
    dev = torch.device(DEV)
    whole_eng = make_engine(cfg, sd, dev)
    e = _a2h_engine(cfg, sd, ff + 2)
    e.bind_multi(4)
    F1 = e.receptive_field - 1
    specs, wholes = [], []
    for k in range(4):
        a = audio[2 * k:]
        nf = a.shape[0] - ff
        specs.append(dict(audio=a, pre=pre, noise=noise[:nf], expq=expq[:nf], slot=k, bounds=list(range(0, F1 + nf + 1))))
        wholes.append(run(whole_eng, cfg, a, pre, noise[:nf], expq[:nf], sigma, ff, dev))
    got = _run_streams(e, cfg, specs, sigma, ff)
    for k in range(4):
        assert np.array_equal(got[k], wholes[k]), "stream %d" % k


@pytest.mark.parametrize("name", ["default_n300", "nc2_l4b1"])
def test_generate_resume_multi_shares_its_state_with_the_single_stream_call(name):
    meta, cfg, sd, audio, pre, ref, noise, expq = load_case(name)
    sigma, ff = meta["sigma_scale"], meta["frame_future"]
    gmm, nc = cfg["loss"] == "GMM", cfg["ncenter"]
    e = _a2h_engine(cfg, sd, audio.shape[0])
    e.bind_multi(2)
    F1 = e.receptive_field - 1
    n = audio.shape[0] - ff
    k = n // 3
    whole = _resume_chain(e, cfg, audio, pre, noise, expq, sigma, ff, [])
    nz = lambda f0, f1: _d(noise[f0:f1]) if gmm else None
    eq = lambda f0, f1: _d(expq[f0:f1]) if gmm and nc > 1 else None
    s0, s1 = (torch.empty(e.state_bytes(), dtype=torch.uint8, device=DEV) for _ in range(2))
    # single -> multi
    a = e.generate_resume(_d(audio[:k + ff]), 0, _d(pre), nz(0, k), eq(0, k), sigma, ff, 0, k, None, s0)
    assert e.status() == 0
    b = e.generate_resume_multi([dict(slot=1, row0=0, n_new=audio.shape[0], step0=F1 + k, step1=F1 + n, noise=nz(k, n), expq=eq(k, n),
                                      state_in=s0, state_out=s1)], _d(audio), sigma, ff)[0]
    assert e.status_multi() == 0
    assert np.array_equal(np.concatenate([a.cpu().numpy(), b.cpu().numpy()]), whole)
    # multi (priming in two slices, then k frames) -> single
    t0, t1 = (torch.empty(e.state_bytes(), dtype=torch.uint8, device=DEV) for _ in range(2))
    e.generate_resume_multi([dict(slot=0, row0=0, n_new=audio.shape[0], step0=0, step1=F1 // 2, pre=_d(pre), state_out=t0)], _d(audio), sigma, ff)
    a = e.generate_resume_multi([dict(slot=0, row0=audio.shape[0], n_new=0, step0=F1 // 2, step1=F1 + k, noise=nz(0, k), expq=eq(0, k),
                                      state_in=t0, state_out=t1)], None, sigma, ff)[0]
    assert e.status_multi() == 0
    b = e.generate_resume(_d(audio), 0, None, nz(k, n), eq(k, n), sigma, ff, k, n - k, t1, t0)
    assert e.status() == 0
    assert np.array_equal(np.concatenate([a.cpu().numpy(), b.cpu().numpy()]), whole)


def test_generate_resume_multi_refusals():
    from livespeechportraits_amd import _native as N
    meta, cfg, sd, audio, pre, ref, noise, expq = load_case("nc2_l4b1")
    sigma, ff = meta["sigma_scale"], meta["frame_future"]
    e = _a2h_engine(cfg, sd, ff + 4)
    with pytest.raises(RuntimeError, match="bind_multi"):
        e.generate_resume_multi([dict(slot=0, step0=0, step1=1, pre=_d(pre))], None, sigma, ff)
    e.bind_multi(3)
    F1 = e.receptive_field - 1
    s0, s1, s2 = (torch.empty(e.state_bytes(), dtype=torch.uint8, device=DEV) for _ in range(3))
    ok = dict(slot=0, row0=0, n_new=1, step0=0, step1=2, pre=_d(pre), state_out=s2)
    with pytest.raises(N.Lspa2hError, match="stream 1: .*not passed"):     # frame 0 (step F1) needs row ff
        e.generate_resume_multi([ok, dict(slot=1, row0=0, n_new=ff, step0=0, step1=F1 + 1, pre=_d(pre), noise=_d(noise[:1]), expq=_d(expq[:1]))],
                                _d(audio[:ff + 1]), sigma, ff)
    with pytest.raises(N.Lspa2hError, match="stream 1: .*step0 must be 0"):
        e.generate_resume_multi([ok, dict(slot=1, row0=0, n_new=1, step0=3, step1=4, pre=_d(pre))], _d(audio[:2]), sigma, ff)
    with pytest.raises(N.Lspa2hError, match="stream 1: .*expq"):
        e.generate_resume_multi([ok, dict(slot=1, row0=0, n_new=ff + 1, step0=0, step1=F1 + 1, pre=_d(pre), noise=_d(noise[:1]))],
                                _d(audio[:ff + 2]), sigma, ff)
    with pytest.raises(N.Lspa2hError, match="stream 1: .*slot"):
        e.generate_resume_multi([ok, dict(ok, state_out=s1)], _d(audio[:2]), sigma, ff)
    with pytest.raises(N.Lspa2hError, match="slot"):
        e.generate_resume_multi([dict(ok, slot=3)], _d(audio[:1]), sigma, ff)
    e.generate_resume_multi([dict(ok, state_out=s0)], _d(audio[:1]), sigma, ff)
    assert e.status_multi() == 0
    with pytest.raises(N.Lspa2hError, match="separate"):
        e.generate_resume_multi([dict(slot=0, row0=1, n_new=0, step0=2, step1=3, state_in=s0, state_out=s0)], None, sigma, ff)
    with pytest.raises(N.Lspa2hError, match="stream 1: .*separate"):       # stream 1 would overwrite the state stream 0 reads
        e.generate_resume_multi([dict(slot=0, row0=1, n_new=0, step0=2, step1=3, state_in=s0, state_out=s1),
                                 dict(slot=1, row0=0, n_new=1, step0=0, step1=1, pre=_d(pre), state_out=s0)], _d(audio[:1]), sigma, ff)
    with pytest.raises(N.Lspa2hError, match="left the projection ring"):   # step 2 reads row 0, overwritten by rows ff+4 ..
        e.generate_resume_multi([dict(slot=0, row0=1, n_new=ff + 4, step0=2, step1=3, state_in=s0, state_out=s1)], _d(audio[1:ff + 5]), sigma, ff)
    # a state that belongs to another step is refused on the device, through the status word: that stream's outputs stay untouched,
    # the other stream of the call is served
    out_bad = torch.full((1, cfg["ndim"]), 7.0, device=DEV)
    good = _a2h_engine(cfg, sd, audio.shape[0])
    good.bind_multi(1)
    want = good.generate_resume_multi([dict(slot=0, row0=0, n_new=audio.shape[0], step0=0, step1=F1 + 1, pre=_d(pre), noise=_d(noise[:1]),
                                            expq=_d(expq[:1]))], _d(audio), sigma, ff)[0].cpu()
    assert good.status_multi() == 0
    s1.fill_(9)
    big = _a2h_engine(cfg, sd, audio.shape[0])
    big.bind_multi(2)
    big.generate_resume_multi([dict(slot=0, row0=0, n_new=1, step0=0, step1=2, pre=_d(pre), state_out=s0)], _d(audio[:1]), sigma, ff)
    outs = big.generate_resume_multi(
        [dict(slot=0, row0=1, n_new=audio.shape[0] - 1, step0=F1, step1=F1 + 1, noise=_d(noise[:1]), expq=_d(expq[:1]), state_in=s0, state_out=s1,
              out=out_bad),                                                # s0 holds the state after step 1, not after step F1 - 1
         dict(slot=1, row0=0, n_new=audio.shape[0], step0=0, step1=F1 + 1, pre=_d(pre), noise=_d(noise[:1]), expq=_d(expq[:1]))],
        _d(np.concatenate([audio[1:], audio])), sigma, ff)
    assert big.status_multi() == 0x5000000
    assert bool((out_bad == 7.0).all()) and bool((s1 == 9).all())
    assert torch.equal(outs[1].cpu(), want)


# ---- mel: windows of several buffers in one call -------------------------------------------------------------------------
def test_mel_ranges_equal_one_range_per_buffer():
    from livespeechportraits_amd import _native as N, mel
    lib = N.load()
    start = lambda i: int(lib.lspmel_window_start(i))
    waves = [torch.from_numpy(wave_of(n, seed=n)).to(DEV) for n in (16000 * 2 + 77, 4000, 267)]
    segs = []
    # buffer 0: windows 30..99 from a buffer that starts a little early and goes on past them; buffer 1: the zero-padded last windows of
    # an ended clip; buffer 2: the whole of a clip of one frame, ended
    f0 = start(30) - 2
    segs.append((waves[0][f0:start(99) + 266 + 31].contiguous(), f0, 30, 70, False))
    n1 = int(lib.lspmel_num_windows(4000))
    f1 = start(n1 - 5)
    segs.append((waves[1][f1:].contiguous(), f1, n1 - 5, 5, True))
    segs.append((waves[2], 0, 0, int(lib.lspmel_num_windows(267)), True))
    assert start(n1 - 1) + 266 > 4000                                       # the last window of buffer 1 really is zero padded
    got = mel.compute_mel_ranges(segs).cpu()
    want = torch.cat([mel.compute_mel_range(*sg).cpu() for sg in segs])
    assert got.shape == want.shape and torch.equal(got, want)
    for k, w in enumerate(waves):                                           # and the whole-clip rows
        whole = mel.compute_mel(w).cpu()
        r0 = sum(s[3] for s in segs[:k])
        assert torch.equal(got[r0:r0 + segs[k][3]], whole[segs[k][2]:segs[k][2] + segs[k][3]])
    # another order, one segment alone
    assert torch.equal(mel.compute_mel_ranges(segs[::-1]).cpu(), torch.cat([want[75:], want[70:75], want[:70]]))
    assert torch.equal(mel.compute_mel_ranges(segs[1:2]).cpu(), want[70:75])
    # per-segment refusals
    with pytest.raises(N.LspmelError, match="segment 1: .*not ended"):
        mel.compute_mel_ranges([segs[0], segs[1][:4] + (False,)])
    with pytest.raises(N.LspmelError, match="segment 2: .*before first_sample"):
        mel.compute_mel_ranges([segs[0], segs[1], (waves[2], 1, 0, 2, True)])
    with pytest.raises(N.LspmelError, match="segment 0: .*past the last one"):
        mel.compute_mel_ranges([(waves[2], 0, 0, 4, True)])
    with pytest.raises(ValueError):
        mel.compute_mel_ranges([segs[0]] * 17)


# ---- the pool ------------------------------------------------------------------------------------------------------------
def pool_of(m, **kw):
    from livespeechportraits_amd.live_pool import LiveSessionPool
    return LiveSessionPool(m["apc"], m["a2f"], m["a2h"], m["db"], True, 10, 1.0, sigma_scale=0.3, device=DEV, feature_opt=m["fopt"],
                           headpose_opt=m["hopt"], **kw)


def _random_pieces(n, seed):
    rng, out = np.random.default_rng(seed), []
    while n:
        out.append(min(n, int(rng.integers(1, 8001))))
        n -= out[-1]
    return out


def _pool_scenario(m, refs, **kw):
    """Five sessions with different clips and chunkings join at different ticks; the one-frame session finishes while the others run and
    a sixth session reopens its slot.  Every session has a generator of its own, seeded like its whole-clip reference."""
    pool = pool_of(m, max_sessions=5, **kw)
    n1, n16, n300 = int(1 * 16000 / 60) + 1, int(16 * 16000 / 60) + 1, int(300 * 16000 / 60) + 1
    plan = [  # (joins at tick, samples, seed, pieces); all five are open from tick 3 on, the one-frame session finishes at tick 5
        (0, CLIP_SAMPLES, 21, [CLIP_SAMPLES] + [0] * 40),                     # whole clip at once, finished 40 empty pushes later
        (1, n1, 22, [n1, 0, 0, 0, 0]),
        (1, n16, 23, frame_pieces(n16)),
        (2, n300, 24, _random_pieces(n300, 9)),
        (3, CLIP_SAMPLES, 25, [1] * 700 + frame_pieces(CLIP_SAMPLES, 700)),
        (6, n16, 26, [n16]),                          # the sixth: joins once the one-frame session has finished, in its slot
    ]
    state, got = {}, {}
    tick = 0
    while len(got) < len(plan):
        for i, (join, n, seed, pieces) in enumerate(plan):
            if i not in state and i not in got and tick >= join and len(pool.open_sessions) < 5:
                sid = pool.open(np.zeros(12, np.float32), generator=torch.Generator().manual_seed(seed))
                state[i] = dict(sid=sid, pos=0, k=0, mouth=[], poses=[], slot=pool.plan.slot[sid])
        push, finish = {}, []
        for i, st in state.items():
            pieces = plan[i][3]
            if st["k"] < len(pieces):
                n = pieces[st["k"]]
                push[st["sid"]] = refs[i][0][st["pos"]:st["pos"] + n]
                st["pos"] += n
                st["k"] += 1
            if st["k"] == len(pieces):
                finish.append(st["sid"])
        out = pool.tick(push, finish=finish, host=True)
        for i in list(state):
            st = state[i]
            o = out.get(st["sid"])
            if o is not None:
                assert o.mouth_start == sum(len(x) for x in st["mouth"]) and o.pose_start == sum(len(x) for x in st["poses"])
                st["mouth"].append(o.mouth)
                st["poses"].append(o.poses)
            if st["sid"] in finish:
                got[i] = (np.concatenate(st["mouth"]), np.concatenate(st["poses"]), st["slot"])
                del state[i]
        tick += 1
    assert got[5][2] == got[1][2], "the sixth session did not reuse the finished session's slot"
    for i in range(len(plan)):
        assert np.array_equal(got[i][0], refs[i][1]), "mouth rows of session %d" % i
        assert np.array_equal(got[i][1].astype(np.float64), refs[i][2]), "poses of session %d" % i
    assert pool.open_sessions == []


@pytest.fixture(scope="module")
def scenario_refs(models):
    n1, n16, n300 = int(1 * 16000 / 60) + 1, int(16 * 16000 / 60) + 1, int(300 * 16000 / 60) + 1
    refs = []
    for n, seed in ((CLIP_SAMPLES, 21), (n1, 22), (n16, 23), (n300, 24), (CLIP_SAMPLES, 25), (n16, 26)):
        wave = wave_of(n, seed=seed)
        mouth, poses = whole_clip(models, wave, seed)
        refs.append((wave, mouth, poses))
    return refs


@pytest.mark.parametrize("kw", [{}, {"max_chunk_samples": 2000}, {"prime_steps_per_tick": 1}, {"prime_steps_per_tick": 254}],
                         ids=["default", "chunk2000", "prime1", "prime254"])
def test_pool_sessions_equal_whole_clip(models, scenario_refs, kw):
    _pool_scenario(models, scenario_refs, **kw)


def test_pool_of_one_equals_front_end(models):
    """LiveAudioFrontEnd is a pool of one, so the comparison with a pool session pins the wrapper's mapping (start indices, finish, the
    generator handed over); the independent leg is the whole-clip path, which the pool session's rows equal bit for bit."""
    wave = wave_of(CLIP_SAMPLES, seed=31)
    ref_mouth, ref_poses = whole_clip(models, wave, seed=5)
    pieces = frame_pieces(16000) + _random_pieces(CLIP_SAMPLES - 16000, 3)
    fe = session(models, generator=torch.Generator().manual_seed(5))
    pool = pool_of(models, max_sessions=1)
    sid = pool.open(np.zeros(12, np.float32), generator=torch.Generator().manual_seed(5))
    pos, mouth, poses = 0, [], []
    for k in pieces:
        a = fe.push(wave[pos:pos + k], host=True)
        b = pool.tick({sid: wave[pos:pos + k]}, host=True)[sid]
        pos += k
        assert (a.mouth_start, a.pose_start) == (b.mouth_start, b.pose_start)
        assert np.array_equal(a.mouth, b.mouth) and np.array_equal(a.poses, b.poses), "at sample %d" % pos
        mouth.append(b.mouth)
        poses.append(b.poses)
    a, b = fe.finish(host=True), pool.tick(finish=[sid], host=True)[sid]
    assert (a.mouth_start, a.pose_start) == (b.mouth_start, b.pose_start)
    assert np.array_equal(a.mouth, b.mouth) and np.array_equal(a.poses, b.poses)
    assert np.array_equal(np.concatenate(mouth + [b.mouth]), ref_mouth)
    assert np.array_equal(np.concatenate(poses + [b.poses]).astype(np.float64), ref_poses)
    # device tensors in, device tensors out
    sid = pool.open(np.zeros(12, np.float32))
    out = pool.tick({sid: torch.from_numpy(wave[:8000]).to(DEV)}, finish=[sid])[sid]
    assert out.mouth.is_cuda and out.mouth.shape == (30, 75) and out.poses.shape == (15, 12)


def test_pool_memory_is_bounded(models):
    wave = wave_of(CLIP_SAMPLES, seed=4)
    pool = pool_of(models, max_sessions=8)
    pieces = frame_pieces(CLIP_SAMPLES)
    sids = [pool.open(np.zeros(12, np.float32)) for _ in range(8)]
    pos = {sid: (0, 0) for sid in sids}

    def tick(rep):
        push = {}
        for sid in list(pos):
            p, k = pos[sid]
            n = pieces[k]
            push[sid] = wave[p:p + n]
            pos[sid] = (p + n, k + 1)
        finish = []
        if rep % 100 == 50:                                                    # a session closes and another opens in its slot
            finish = [sorted(pos)[0]]
        for sid in list(pos):
            if pos[sid][1] >= len(pieces) and sid not in finish:
                finish.append(sid)
        pool.tick(push, finish=finish)
        for sid in finish:
            del pos[sid]
            pos[pool.open(np.zeros(12, np.float32))] = (0, 0)

    for rep in range(40):
        tick(rep)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for rep in range(40, 1040):
        tick(rep)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base


def test_pool_refusals(models, tmp_path):
    import argparse
    import os
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.live_pool import LiveSessionPool
    from livespeechportraits_amd.models import create_model
    pool = pool_of(models, max_sessions=2)
    a, b = pool.open(np.zeros(12, np.float32)), pool.open(np.zeros(12, np.float32))
    with pytest.raises(RuntimeError, match="max_sessions"):
        pool.open(np.zeros(12, np.float32))
    with pytest.raises(ValueError):
        pool.tick({a: np.zeros(100, np.float64)})
    with pytest.raises(ValueError):
        pool.tick({a: np.zeros((2, 100), np.float32)})
    with pytest.raises(ValueError):
        pool.tick({a: torch.zeros(100, dtype=torch.float16, device=DEV)})
    with pytest.raises(KeyError):
        pool.tick({77: np.zeros(100, np.float32)})
    with pytest.raises(ValueError, match="twice"):
        pool.tick([(a, np.zeros(10, np.float32)), (a, np.zeros(10, np.float32))])
    with pytest.raises(ValueError, match="twice"):
        pool.tick({a: np.zeros(10, np.float32)}, finish=[b, b])
    assert pool.plan.sched[a].n_samples == 0 and pool.plan.sched[b].n_samples == 0     # a refused tick changes nothing
    pool.tick({a: torch.zeros(100, device=DEV), b: np.zeros(50, np.float32)}, finish=[a])
    with pytest.raises(RuntimeError, match="closed"):                         # pushed after its finish
        pool.tick({a: np.zeros(1, np.float32)})
    with pytest.raises(RuntimeError, match="closed"):
        pool.tick(finish=[a])
    with pytest.raises(RuntimeError, match="closed"):
        pool.close(a)
    pool.close(b)
    with pytest.raises(RuntimeError, match="GPU"):
        LiveSessionPool(models["apc"], models["a2f"], models["a2h"], models["db"], True, 10, 1.0, device="cpu")
    with pytest.raises(ValueError):
        pool_of(models, max_sessions=17)
    ck = os.path.join(str(tmp_path), "Audio2Headpose.pkl")
    torch.save({"module." + k: torch.from_numpy(v) for k, v in synth.make_a2h_lstm_state_dict(512, 1, 12, "GMM").items()}, ck)
    lopt = argparse.Namespace(model="audio2headpose", gpu_ids=[0], isTrain=False, checkpoints_dir=str(tmp_path), name="x", load_epoch=ck,
                              verbose=False, feature_decoder="LSTM", loss="GMM", A2H_GMM_ndim=12, A2H_GMM_ncenter=1, APC_hidden_size=512,
                              frame_future=15)
    lstm = create_model(lopt)
    lstm.setup(lopt)
    with pytest.raises(NotImplementedError, match="LSTM"):
        LiveSessionPool(models["apc"], models["a2f"], lstm, models["db"], True, 10, 1.0, device=DEV, feature_opt=models["fopt"], headpose_opt=lopt)

    class Residual:
        rnn_residual = True
    with pytest.raises(NotImplementedError, match="residual"):
        LiveSessionPool(Residual(), models["a2f"], models["a2h"], models["db"], True, 10, 1.0, device=DEV)


def test_pool_real_time(models):
    """16 sessions opened two ticks apart, each pushed one frame of audio per tick over the 687-frame clip, with the feature database of
    bench.py's pipeline (30 000 rows).  The whole pool's tick (call -> frames of all sessions on the host) must fit a frame time, 1/60 s:
    the bound of test_session_real_time, derived from demo.py's 60 fps.  The other way of serving 16 streams -- 16 pools of one
    (LiveAudioFrontEnd objects) pushed one after another -- is timed in the same process; only the direction is asserted."""
    from livespeechportraits_amd import synth
    m = dict(models, db=synth.make_feature_database(30000, 8, 512, 24)[0])
    wave = wave_of(CLIP_SAMPLES, seed=11)
    pieces = frame_pieces(CLIP_SAMPLES)
    S = 16

    def serve(push_all, open_one, finish_one):
        """tick t: session j (opened at tick 2j) pushes its piece t - 2j"""
        ts, live = [], {}
        for t in range(len(pieces) + 2 * (S - 1)):
            if t % 2 == 0 and t // 2 < S:
                live[t // 2] = open_one()
            work = [(j, t - 2 * j) for j in sorted(live) if 0 <= t - 2 * j < len(pieces)]
            t0 = time.perf_counter()
            push_all([(live[j], k) for j, k in work])
            ts.append(time.perf_counter() - t0)
            for j, k in work:
                if k == len(pieces) - 1:
                    finish_one(live.pop(j))
        return np.array(ts)

    starts = np.concatenate([[0], np.cumsum(pieces)])
    piece = lambda k: wave[starts[k]:starts[k + 1]]
    pool = pool_of(m, max_sessions=S)
    tp = serve(lambda work: pool.tick({sid: piece(k) for sid, k in work}, host=True),
               lambda: pool.open(np.zeros(12, np.float32)), lambda sid: pool.tick(finish=[sid]))
    fes = serve(lambda work: [fe.push(piece(k), host=True) for fe, k in work], lambda: session(m), lambda fe: fe.finish())
    full = slice(2 * (S - 1), len(pieces))                                    # the ticks in which all 16 sessions push
    p50, p99 = np.percentile(tp, 50), np.percentile(tp, 99)
    q50, q99 = np.percentile(fes[full], 50), np.percentile(fes[full], 99)
    print("\n[live pool] 16 sessions, tick: p50 %.3f ms, p99 %.3f ms, max %.3f ms (ticks with all 16: p50 %.3f ms)"
          % (p50 * 1e3, p99 * 1e3, tp.max() * 1e3, np.percentile(tp[full], 50) * 1e3))
    print("[live pool] 16 pools of one (LiveAudioFrontEnd) one after another, ticks with all 16: p50 %.3f ms, p99 %.3f ms, max %.3f ms; ratio of the p50s %.2f"
          % (q50 * 1e3, q99 * 1e3, fes[full].max() * 1e3, q50 / np.percentile(tp[full], 50)))
    assert p99 < 1.0 / 60
    assert np.percentile(tp[full], 50) < q50
