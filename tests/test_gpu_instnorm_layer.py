"""InstanceNorm, layer by layer: the standalone passes (lspf2f_instance_norm: in_small; in_reduce_stats -> in_finalize -> in_apply) and the four fused
statistics producers (lspf2f_conv3x3_instnorm: the implicit GEMM's epilogue sums, wino3x3, winoup3x3, the tiny-M kernel) against numpy float64, at the
shapes where the kernels take another path and on channels with |mean| >> std, constant channels, one odd row, and a ramp across the groups.

The tolerance is derived, not tuned: the best ANY fp32 InstanceNorm can do on a channel is floor = rstd * ulp32(|mean|) / 2 + 2^-23 (1 + max|y|) (the mean
rounded to fp32, amplified; then the subtraction, product and residual-add roundings); the kernels are held to 4 x that, per channel.  The CPU model of
the same arithmetic (tests/instnorm_model.py, tests/test_instnorm_model_cpu.py) stays inside it on every case here and three wrong kernels do not.  The
worst measured err / floor per route and producer is printed by the last test of this file."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import instnorm_model as M

pytestmark = pytest.mark.gpu

FACTOR = 4.0
WORST = {}                    # route / producer -> (err / floor, case)


def note(route, ratio, case):
    if ratio >= WORST.get(route, (-1.0, None))[0]:
        WORST[route] = (ratio, case)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def instance_norm(dev, x, residual, relu, route, partial=None, bias=None, three_pass=0, stats=False, shape=None):
    """x [B][hw][C] fp32 numpy (None with partials [splits][B][hw][C]: the buffer then starts as NaN) -> (y, mean | None, rstd | None) as numpy"""
    from livespeechportraits_amd import _native as N
    lib = N.load()
    b, hw, c = shape if shape is not None else x.shape
    dx = torch.from_numpy(x).to(dev) if x is not None else torch.full((b, hw, c), float("nan"), device=dev)
    dp = torch.from_numpy(partial).to(dev) if partial is not None else None
    db = torch.from_numpy(bias).to(dev) if bias is not None else None
    dr = torch.from_numpy(residual).to(dev) if residual is not None else None
    mean = torch.full((b, c), float("nan"), device=dev) if stats else None
    rstd = torch.full((b, c), float("nan"), device=dev) if stats else None
    sb = lib.lspf2f_instance_norm_scratch_bytes(b, hw, c, route)
    assert sb == (((hw + 63) // 64 * 3 + 2) * b * c * 4 if route == 1 else 0)
    scratch = torch.full((max(sb, 4) // 4,), float("nan"), device=dev)
    N.check(lib.lspf2f_instance_norm(ptr(dx), ptr(dp), 1 if partial is None else partial.shape[0], ptr(db), ptr(dr), int(relu), b, hw, c, route, three_pass,
                                     ptr(mean), ptr(rstd), ptr(scratch), sb, stream()))
    torch.cuda.synchronize()
    return dx.cpu().numpy(), (mean.cpu().numpy() if stats else None), (rstd.cpu().numpy() if stats else None)


def check_against_float64(y, x64, residual, relu, route, case):
    """per (frame, channel): |y - y64| <= 4 floor.  x64 [B][hw][C] float64; returns the float64 (mean, var) [B][C]"""
    assert np.isfinite(y).all(), "unwritten or non-finite outputs"
    means, vars_ = [], []
    for b in range(x64.shape[0]):
        y64, mean64, var64 = M.reference64(x64[b], residual[b] if residual is not None else None, relu)
        err = np.abs(y[b].astype(np.float64) - y64).max(0)
        floor = M.floor32(y64, mean64, var64)
        ratio = float((err / floor).max())
        note(route, ratio, case)
        print("%s %s frame %d: worst err / floor %.2f (channel %d)" % (route, case, b, ratio, int((err / floor).argmax())))
        assert (err <= FACTOR * floor).all(), (case, b, ratio)
        means.append(mean64)
        vars_.append(var64)
    return np.stack(means), np.stack(vars_)


# ---- the standalone passes ------------------------------------------------------------------------------------------------------------------
def standalone_cases():
    """a covering set, not the product: every hw once with the channel counts in rotation, the instance / group boundaries again at the other channel counts,
    split-K partials + bias at ragged extents.  (route, B, hw, C, splits, residual, relu, family offset)"""
    small_hw = (4, 9, 31, 32, 33, 64, 65, 144, 256, 257, 576, 1024, 1025)
    small_c = (4, 32, 96, 160)
    cases = []
    for i, hw in enumerate(small_hw):
        cases.append((0, 3 if i % 2 else 1, hw, small_c[i % 4], 1, i % 2 == 0, i % 3 == 0, i))
    for i, (hw, c) in enumerate([(32, 96), (33, 4), (64, 160), (65, 32), (256, 4), (257, 96), (1024, 160), (1025, 32), (1024, 4), (576, 96)]):
        cases.append((0, 1 if i % 2 else 3, hw, c, 1, i % 2 == 1, i % 3 == 1, i + 2))
    for i, (hw, c) in enumerate([(9, 4), (33, 96), (257, 32), (1025, 160)]):
        cases.append((0, 3 if i % 2 else 1, hw, c, 3, i % 2 == 0, i % 2 == 1, i + 4))
    for i, (hw, c) in enumerate([(1, 96), (63, 96), (64, 96), (65, 96), (1296, 96), (4097, 96), (1296, 4), (1296, 160), (1296, 1024), (4097, 4), (4097, 160), (4097, 1024),
                                 (65, 4), (65, 1024), (1, 1024), (63, 4), (64, 160), (1, 4)]):
        cases.append((1, 3 if i % 2 and hw * c < 2 ** 21 else 1, hw, c, 1, i % 2 == 0, i % 3 == 0, i))
    for i, (hw, c) in enumerate([(1296, 96), (65, 160), (4097, 4), (63, 1024)]):
        cases.append((1, 3 if i % 2 else 1, hw, c, 3, i % 2 == 1, i % 2 == 0, i + 5))
    return cases


def case_id(c):
    return "%s_b%d_hw%d_c%d_k%d%s%s" % (("small", "reduce")[c[0]], c[1], c[2], c[3], c[4], "_res" if c[5] else "", "_relu" if c[6] else "")


@pytest.mark.parametrize("case", standalone_cases(), ids=case_id)
def test_standalone_passes_against_float64(case, gpu_device):
    route, b, hw, c, splits, has_res, relu, offset = case
    name = ("in_small", "reduce")[route]
    rng = np.random.default_rng(7919 * hw + 31 * c + 3 * b + splits + route)
    x = np.stack([M.make_input(rng, hw, c, offset + f) for f in range(b)])
    res = rng.standard_normal((b, hw, c)).astype(np.float32) if has_res else None
    partial = bias = None
    if splits > 1:
        # partials that add up to the family's tensor (to fp32 rounding); the reference is the float64 sum of what the kernel is given
        partial, bias, x64 = M.split_partials(rng, x, splits)
        run = lambda **kw: instance_norm(gpu_device, None, res, relu, route, partial, bias, shape=(b, hw, c), **kw)
    else:
        x64 = x.astype(np.float64)
        run = lambda **kw: instance_norm(gpu_device, x, res, relu, route, **kw)
    y, mean, rstd = run(stats=route == 1)                    # x is NaN on entry when it is to be folded from the partials: what comes back is the normalised tensor
    mean64, var64 = check_against_float64(y, x64, res, relu, name, case_id(case))
    if route == 1:
        assert np.isfinite(mean).all() and np.isfinite(rstd).all()
        assert (np.abs(mean - mean64) <= M.ulp32(mean64)).all(), np.abs(mean - mean64).max()
        r64 = 1.0 / np.sqrt(var64 + M.EPS)
        rel = np.abs(rstd - r64) / r64
        assert (rel <= M.rstd_rel_bound(var64)).all(), rel.max()
    assert np.array_equal(run()[0], y)                       # fixed order: the same bits again
    if route == 0 and hw <= 1024:
        assert np.array_equal(run(three_pass=1)[0], y)       # rows in registers or re-read from memory: the same operations in the same order
    if b > 1:                                                # statistics are per frame
        for f in range(b):
            one = instance_norm(gpu_device, None if splits > 1 else x[f:f + 1], res[f:f + 1] if has_res else None, relu, route,
                                np.ascontiguousarray(partial[:, f:f + 1]) if splits > 1 else None, bias, shape=(1, hw, c))[0]
            assert np.array_equal(one[0], y[f]), f


def test_standalone_refusals(gpu_device):
    from livespeechportraits_amd import _native as N
    lib = N.load()
    x = torch.zeros(1, 64, 1028, device=gpu_device)
    big = torch.zeros(1 << 20, device=gpu_device)

    def call(xp, hw, c, route, mean=None, scratch_bytes=None):
        sb = big.numel() * 4 if scratch_bytes is None else scratch_bytes
        rc = lib.lspf2f_instance_norm(xp, None, 1, None, None, 0, 1, hw, c, route, 0, mean, None, ptr(big), sb, stream())
        return rc, lib.lspf2f_last_error().decode()

    for route in (0, 1):
        rc, msg = call(ptr(x), 64, 6, route)                 # C % 4 != 0
        assert rc == -2 and "multiple of 4" in msg
        rc, msg = call(ptr(x), 0, 32, route)                 # hw < 1
        assert rc == -2 and "hw" in msg
        rc, msg = call(None, 64, 32, route)                  # null x
        assert rc == -1 and "null x" in msg
    rc, msg = call(ptr(x), 64, 1028, 1)                      # 257 channel quads
    assert rc == -2 and "1024 channels" in msg
    need = lib.lspf2f_instance_norm_scratch_bytes(1, 64, 32, 1)
    rc, msg = call(ptr(x), 64, 32, 1, scratch_bytes=need - 4)
    assert rc != 0 and "scratch" in msg
    rc, msg = call(ptr(x), 64, 32, 0, mean=ptr(big))         # the one-launch route has no statistics to hand out
    assert rc == -1 and "mean_out" in msg
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0 and float(big.abs().sum()) == 0.0      # nothing was launched


# ---- the fused statistics producers -----------------------------------------------------------------------------------------------------------
def conv_problem(b, c0, c1, cout, hs, ho, seed, residual):
    """weights with a few near-constant, large-mean output channels: bias + 8 and the channel's weights x 1e-3"""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(b, c0, hs, hs, generator=g)
    x1 = torch.randn(b, c1, hs, hs, generator=g) if c1 else None
    w = torch.randn(cout, c0 + c1, 3, 3, generator=g) / (3.0 * (c0 + c1) ** 0.5)
    bias = torch.randn(cout, generator=g) * 0.1
    flat = list(range(1, cout, 5))
    w[flat] *= 1e-3
    bias[flat] += 8.0
    res = torch.randn(b, cout, ho, ho, generator=g) if residual else None
    return x0, x1, w, bias, res


def conv_instnorm(dev, x0, x1, w, bias, res, stride, up, relu, tile, split_k, k_group, pack):
    """lspf2f_conv3x3_instnorm on NCHW cpu tensors -> NCHW cpu tensor; `pack` = the weight layout of the kernel behind `tile`"""
    from livespeechportraits_amd import _native as N
    lib = N.load()
    b, c0, hs, _ = x0.shape
    c1 = x1.shape[1] if x1 is not None else 0
    cout = w.shape[0]
    ho = 2 * hs if up else (hs + stride - 1) // stride
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev) if t is not None else None
    d0, d1, dres, wp, db = nhwc(x0), nhwc(x1), nhwc(res), pack(w).to(dev), bias.to(dev)
    out = torch.full((b, ho, ho, cout), float("nan"), device=dev)
    sb = lib.lspf2f_conv3x3_scratch_bytes(b, hs, hs, c0, c1, cout, stride, int(up), tile[0], tile[1], split_k, k_group, 0)
    scratch = torch.zeros(max(sb, 4), dtype=torch.uint8, device=dev)                  # split-K slabs + arrival counters: zero on entry
    nb = lib.lspf2f_conv3x3_instnorm_scratch_bytes(b, hs, hs, c0, c1, cout, stride, int(up), tile[0], tile[1], split_k, k_group, 0)
    stats = torch.full((max(nb, 4) // 4,), float("nan"), device=dev)                  # (a refused selection has no size: the call below says why)
    N.check(lib.lspf2f_conv3x3_instnorm(ptr(d0), ptr(d1), ptr(wp), ptr(db), ptr(dres), ptr(out), b, hs, hs, c0, c1, cout, stride, int(up), int(relu),
                                        tile[0], tile[1], split_k, k_group, 0, ptr(scratch), scratch.numel(), ptr(stats), nb, stream()))
    torch.cuda.synchronize()
    assert nb >= cout * 4
    if sb:
        assert int(scratch[-4:].view(torch.int32).item()) == 0                        # the last arrival counter is back at zero
    return out.permute(0, 3, 1, 2).contiguous().cpu()


def check_fused(got, raw, res, relu, producer, case):
    """got, raw, res: NCHW cpu tensors; the float64 InstanceNorm of the conv's own raw output is the reference"""
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).numpy() if t is not None else None
    assert torch.isfinite(raw).all()
    check_against_float64(rows(got), rows(raw).astype(np.float64), rows(res), relu, producer, case)


IGEMM_CASES = [(2, 32, cout, 32, 0, tile) for cout in (32, 96) for tile in ((128, 64), (64, 64), (32, 64))] + [(2, 32, 32, 32, 2, (64, 64)), (1, 32, 96, 32, 2, (128, 64))]


@pytest.mark.parametrize("cfg", IGEMM_CASES, ids=lambda c: "b%d_c%d_o%d_h%d_up%d_t%dx%d" % (c[:5] + c[5]))
def test_igemm_epilogue_sums(cfg, gpu_device):
    """The implicit GEMM with epilogue sums (one group per wave; the sub-pixel up-conv form has four times the groups) -> in_finalize -> in_apply, against the float64
    InstanceNorm of the raw output the same kernel selection writes through lspf2f_conv3x3 (scale 1, shift = bias): the same launch but for the sums, the same bits."""
    from test_gpu_conv import pack_subpixel, run_conv
    b, c0, cout, hs, up, tile = cfg
    ho = 2 * hs if up else hs
    x0, x1, w, bias, res = conv_problem(b, c0, 0, cout, hs, ho, 100 + cout + tile[0] + up, residual=tile[0] != 64)
    relu = tile[0] != 32
    raw = run_conv(gpu_device, x0, None, w, torch.ones(cout), bias, None, 1, up, False, tile, 1, 0)
    pack = pack_subpixel if up == 2 else (lambda t: t.permute(0, 2, 3, 1).contiguous())
    got = conv_instnorm(gpu_device, x0, None, w, bias, res, 1, up, relu, tile, 1, 0, pack)
    check_fused(got, raw, res, relu, "igemm(stats)", "o%d_up%d_t%dx%d" % (cout, up, tile[0], tile[1]))
    assert torch.equal(conv_instnorm(gpu_device, x0, None, w, bias, res, 1, up, relu, tile, 1, 0, pack), got)


WINO_IN_CASES = [(1, 32, 16, 1, 1), (2, 32, 32, 3, 2), (1, 64, 16, 2, 1), (2, 64, 32, 2, 2), (1, 64, 32, 1, 2), (2, 32, 16, 3, 1), (1, 64, 16, 3, 2), (1, 32, 32, 1, 1),
                 (1, 32, 16, 1, 2), (1, 64, 32, 3, 1)]


@pytest.mark.parametrize("cfg", WINO_IN_CASES, ids=lambda c: "b%d_c%d_h%d_nb%d_s%d" % c)
def test_wino_tile_block_sums(cfg, gpu_device):
    """wino3x3 leaving one group of sums per tile-block of 128 pixels, from its epilogue (one K slice) or from its split-K combine (two), -> in_finalize -> in_apply"""
    from test_gpu_conv import pack_wino, run_wino
    b, c, hs, nb, splits = cfg
    x0, _, w, bias, res = conv_problem(b, c, 0, c, hs, hs, 200 + c + hs + nb + splits, residual=nb != 2)
    relu = splits == 1
    raw = run_wino(gpu_device, x0, w, torch.ones(c), bias, None, False, nb, splits)
    got = conv_instnorm(gpu_device, x0, None, w, bias, res, 1, 0, relu, (4000 + nb, 0), splits, -1, pack_wino)
    check_fused(got, raw, res, relu, "wino3x3(stats)", "c%d_h%d_nb%d_s%d" % (c, hs, nb, splits))
    assert torch.equal(conv_instnorm(gpu_device, x0, None, w, bias, res, 1, 0, relu, (4000 + nb, 0), splits, -1, pack_wino), got)


@pytest.mark.parametrize("nb", [1, 2])
def test_winoup_tile_block_sums(nb, gpu_device):
    """winoup3x3 (the smallest shape of WINOUP_CASES: 8x8 -> 16x16, two groups of 128 output pixels per frame) -> in_finalize -> in_apply"""
    from test_gpu_conv import WINOUP_CASES, run_winoup
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import wino_model
    b, c0, c1, _, hs = WINOUP_CASES[0][:5]
    cout = 32 * nb
    x0, x1, w, bias, res = conv_problem(b, c0, c1, cout, hs, 2 * hs, 300 + nb, residual=nb == 1)
    raw = run_winoup(gpu_device, x0, x1, w, torch.ones(cout), bias, False, nb, 1)
    pack = lambda t: torch.from_numpy(wino_model.pack_u_up(t.numpy()))
    got = conv_instnorm(gpu_device, x0, x1, w, bias, res, 1, 1, nb == 2, (5000 + nb, 0), 1, -1, pack)
    check_fused(got, raw, res, nb == 2, "winoup3x3(stats)", "nb%d" % nb)


@pytest.mark.parametrize("hs", [2, 4])
def test_tiny_m_kernel_normalises_in_its_epilogue(hs, gpu_device):
    """conv3x3_smallm with in_fused = 1 (the 2x2 and 4x4 rows of TINY_CASES: 512 -> 512 channels, statistics over 4 and 16 values), against the float64 InstanceNorm
    of the raw output the same kernel writes without it"""
    from test_gpu_conv import TINY_CASES, run_conv
    b, cin, cout = [c for c in TINY_CASES if c[3] == hs and c[4] == 1 and not c[5]][0][:3]
    x0, _, w, bias, res = conv_problem(b, cin, 0, cout, hs, hs, 400 + hs, residual=hs == 4)
    raw = run_conv(gpu_device, x0, None, w, torch.ones(cout), bias, None, 1, 0, False, (1, 1))
    got = conv_instnorm(gpu_device, x0, None, w, bias, res, 1, 0, True, (1, 1), 0, 0, lambda t: t.permute(0, 2, 3, 1).contiguous())
    check_fused(got, raw, res, True, "smallm(in)", "h%d" % hs)


def test_fused_entry_refuses_everything_else(gpu_device):
    from livespeechportraits_amd import _native as N
    x0, _, w, bias, _ = conv_problem(1, 32, 0, 32, 16, 16, 1, False)
    rows = lambda t: t.permute(0, 2, 3, 1).contiguous()
    for tile, split, kg, why in (((64, 64), 1, 0, "1024 pixels"),          # a 16x16 frame: the planner sends it to in_small
                                 ((16, 16), 0, 0, "producers"),             # the full-K kernel gathers no statistics
                                 ((6001, 0), 1, -1, "producers"),           # nor does wino4_3x3
                                 ((64, 128), 1, 0, "producers"),
                                 ((0, 0), 0, 0, "producers")):
        with pytest.raises(N.Lspf2fError, match=why):
            conv_instnorm(gpu_device, x0, None, w, bias, None, 1, 0, False, tile, split, kg, rows)
    x0, _, w, bias, _ = conv_problem(1, 32, 0, 32, 32, 32, 2, False)
    with pytest.raises(N.Lspf2fError, match="split_k 1"):                   # split-K layers go through in_reduce_stats
        conv_instnorm(gpu_device, x0, None, w, bias, None, 1, 0, False, (64, 64), 2, 0, rows)


def test_zz_report_worst_ratios():
    """the figures DESIGN.md section 14 quotes"""
    for route, (ratio, case) in sorted(WORST.items()):
        print("WORST err / floor  %-18s %.2f  (%s)" % (route, ratio, case))
        assert ratio <= FACTOR
