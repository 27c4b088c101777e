"""conv3x3_smallm's static-geometry instances (one frame of 4x4 -> 4x4, 4x4 -> 2x2 stride 2, 2x2 -> 2x2, 2x2 -> 4x4 upsampled; Cin 256 | 512; fp32):
input pixels held in registers, the tap -> pixel map a compile-time table, both output channels of a workgroup in one packed chain.  They must return
the bits of the run-time-geometry form (tune key smallm_static = 0; k_group bit 0 of lspf2f_conv3x3's tile 1 x 1), which every other shape keeps.

The kernel takes Cin in {256, 512} only (Cin % 256 == 0 and 9 Cin / 4 <= 1280), and both have static instances: "a Cin without a static instance" does not exist at
the entry, so the fallback is exercised by geometry (two frames, a 3x3 input) and by the switch.

The CPU half (no `gpu` mark on those tests): the compile-time tap table, restated in numpy from smallm_geo_pix, against the run-time table formula of the kernel for
every (tap, output pixel) of the four geometries.
"""
import numpy as np
import pytest
import torch

GEOS = {
    # name: (hs, stride, up)      -> ho
    "4to4": (4, 1, False),
    "4to2_s2": (4, 2, False),
    "2to2": (2, 1, False),
    "2to4_up": (2, 1, True),
}
CHANNELS = [(256, 4), (512, 6)]        # (Cin, Cout): the smallest Cin (two workgroups), and the plans' C4 = 128 mapping with a Cout that is no multiple of 4
TOL = 2e-5                             # test_gpu_conv.test_conv3x3_tiny_m_kernel's bound, at its input ranges (|x| <= 1, |w| <= 0.05)
_cache = {}


def _sym(shape, amp, stream):
    from livespeechportraits_amd import synth
    n = int(np.prod(shape))
    return torch.from_numpy(synth.symmetric(n, amp / np.sqrt(3.0), stream).reshape(shape).copy())


def problem(b, cin, cout, hs, stride, up):
    """seeded inputs and the float64 convolution (raw: before scale / shift / residual / ReLU are applied by ref_conv), computed once per shape"""
    key = (b, cin, cout, hs, stride, up)
    if key not in _cache:
        ho = 2 * hs if up else (hs + stride - 1) // stride
        _cache[key] = dict(x=_sym((b, cin, hs, hs), 1.0, 101), w=_sym((cout, cin, 3, 3), 0.05, 102), scale=_sym((cout,), 0.5, 103) + 1.0,
                           shift=_sym((cout,), 0.1, 104), res=_sym((b, cout, ho, ho), 1.0, 105))
    return _cache[key]


def run(dev, pr, stride, up, bn, res, relu, form):
    """form = k_group of the tile 1 x 1 code: bit 0 the run-time-geometry kernel, bit 1 the prefetch wave"""
    from test_gpu_conv import run_conv
    return run_conv(dev, pr["x"], None, pr["w"], pr["scale"] if bn else None, pr["shift"] if bn else None, pr["res"] if res else None, stride, int(up), relu, (1, 1), 0, form)


# ---- CPU: the compile-time tap table against the run-time formula ----
def static_pix(geo, tap, m):
    """smallm_geo_pix (small_layers.hip): geometry 1..4 in GEOS' order; -1 = a padding tap"""
    hs = 4 if geo in (1, 2) else 2
    ho = 4 if geo in (1, 4) else 2
    stride, up = (2 if geo == 2 else 1), geo == 4
    oy, ox = divmod(m, ho)
    uy, ux = oy * stride + tap // 3 - 1, ox * stride + tap % 3 - 1
    hl = 2 * hs if up else hs
    if uy < 0 or uy >= hl or ux < 0 or ux >= hl:
        return -1
    return (uy >> 1 if up else uy) * hs + (ux >> 1 if up else ux)


def runtime_pixtab(B, Hs, Ws, Ho, Wo, stride, up, M, MM):
    """the kernel's step 2, thread by thread: pixtab[t * MM + m], padding and rows past M -> the zero pixel B * Hs * Ws"""
    tab = np.empty(9 * MM, np.int64)
    for tid in range(9 * MM):
        t, m = divmod(tid, MM)
        pix = B * Hs * Ws
        if m < M:
            b, r = divmod(m, Ho * Wo)
            oy, ox = divmod(r, Wo)
            uy, ux = oy * stride + t // 3 - 1, ox * stride + t % 3 - 1
            hl, wl = (2 * Hs, 2 * Ws) if up else (Hs, Ws)
            if 0 <= uy < hl and 0 <= ux < wl:
                pix = (b * Hs + (uy >> 1 if up else uy)) * Ws + (ux >> 1 if up else ux)
        tab[tid] = pix
    return tab


def test_static_tap_tables_equal_the_runtime_table():
    for geo, (hs, stride, up) in enumerate(GEOS.values(), 1):
        ho = 2 * hs if up else hs // stride
        mm = ho * ho
        tab = runtime_pixtab(1, hs, hs, ho, ho, stride, up, mm, mm)
        live = 0
        for tap in range(9):
            for m in range(mm):
                want = tab[tap * mm + m]
                got = static_pix(geo, tap, m)
                assert got == (want if want < hs * hs else -1), (geo, tap, m)
                live += got >= 0
        # (stride 1 over h x h: (3h - 2)^2 live taps; stride 2 from 4x4: 25; the up-conv gathers as a 4x4 stride-1 conv does)
        assert live == {1: 100, 2: 25, 3: 16, 4: 100}[geo]


def test_the_taps_of_a_thread_group_cover_each_tap_once():
    """taps tid / C4 + (256 / C4) j for j < 5, kept while < 9 (the run-time form's k4 < K4): every tap exactly once over the groups, for both channel counts"""
    for c4 in (64, 128):
        seen = sorted(g + (256 // c4) * j for g in range(256 // c4) for j in range(5) if g + (256 // c4) * j < 9)
        assert seen == list(range(9))
        for tid in range(256):
            for j in range(5):
                k4 = tid + 256 * j
                if k4 < 9 * c4:
                    assert (k4 // c4, k4 % c4) == (tid // c4 + (256 // c4) * j, tid % c4)


def test_static_instances_fit_the_register_file(tmp_path):
    """A static instance holds 16 input quads, 10 weight quads and 16 accumulator pairs per lane.  With the prefetch wave a workgroup is five waves, so two share a SIMD:
    <= 256 registers per lane and no scratch, read off the compiler's resource report (as test_wino_cpu does for the Winograd kernels); all 16 instances are built."""
    import os
    import re
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(root, "livespeechportraits_amd", "csrc", "small_layers.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "s.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    static = set()
    for b in re.split(r"remark: Function Name: ", p.stderr)[1:]:
        name = b.split()[0]
        m = re.search(r"conv3x3_smallmIfLi2ELb([01])ELi(\d+)ELb0ELi([1-4])ELi(\d+)E", name)
        if not m:
            continue
        static.add(tuple(int(g) for g in m.groups()))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        vgpr = int(re.search(r" VGPRs: (\d+)", b).group(1))
        agpr = int(re.search(r"AGPRs: (\d+)", b).group(1))
        assert scratch == 0 and vgpr + agpr <= 256, (name, scratch, vgpr, agpr)
    assert static == {(pf, 16 if geo in (1, 4) else 4, geo, c4) for pf in (0, 1) for geo in (1, 2, 3, 4) for c4 in (64, 128)}, sorted(static)


# ---- GPU ----
@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout", CHANNELS, ids=lambda v: str(v))
@pytest.mark.parametrize("geo", list(GEOS))
def test_static_instance_returns_the_bits_of_the_runtime_form(geo, cin, cout, gpu_device):
    from test_gpu_conv import ref_conv
    hs, stride, up = GEOS[geo]
    pr = problem(1, cin, cout, hs, stride, up)
    for bn, res, relu in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        old = run(gpu_device, pr, stride, up, bn, res, relu, 1)
        new = run(gpu_device, pr, stride, up, bn, res, relu, 0)
        assert torch.isfinite(new).all() and torch.equal(new, old), (geo, bn, res, relu, (new - old).abs().max().item())
        ref = ref_conv(pr["x"], None, pr["w"], pr["scale"] if bn else None, pr["shift"] if bn else None, pr["res"] if res else None, stride, up, relu)
        assert new.shape == ref.shape and (new - ref).abs().max().item() <= TOL
    # with the prefetch wave (its own instances): the same bits, from both forms, and again on a repeat
    base = run(gpu_device, pr, stride, up, True, True, True, 1)
    for form in (2, 2, 3):
        assert torch.equal(run(gpu_device, pr, stride, up, True, True, True, form), base), (geo, form)
    assert torch.equal(run(gpu_device, pr, stride, up, True, True, True, 0), base)


@pytest.mark.gpu
@pytest.mark.parametrize("b,cin,cout,hs,stride,up", [(2, 256, 4, 2, 1, False), (1, 256, 4, 3, 1, False), (1, 512, 6, 1, 1, True), (4, 512, 6, 2, 1, False)],
                         ids=lambda v: str(int(v)))
def test_other_shapes_keep_the_runtime_form(b, cin, cout, hs, stride, up, gpu_device):
    """two frames at 2x2, a 3x3 input, a 1x1 source upsampled to 2x2, four frames (16 pixels): no static instance, so both codes run the same kernel"""
    from test_gpu_conv import ref_conv
    pr = problem(b, cin, cout, hs, stride, up)
    new = run(gpu_device, pr, stride, up, True, True, True, 0)
    assert torch.equal(new, run(gpu_device, pr, stride, up, True, True, True, 1))
    assert torch.equal(new, run(gpu_device, pr, stride, up, True, True, True, 2))
    ref = ref_conv(pr["x"], None, pr["w"], pr["scale"], pr["shift"], pr["res"], stride, up, True)
    assert (new - ref).abs().max().item() <= TOL


@pytest.mark.gpu
def test_one_frame_large_forward_is_bit_identical(gpu_device):
    """`large`, one frame (the smallest size the network tests use): smallm_static = 1 against 0, and the switch takes 0 or 1 only"""
    from conftest import golden_problem
    from livespeechportraits_amd import _native as N
    from livespeechportraits_amd.engine import Engine
    meta, arrays, topo, sd, feat, cand = golden_problem("large_s128_b2")
    f, c = torch.from_numpy(feat[:1].copy()).to(gpu_device), torch.from_numpy(cand[:1].copy()).to(gpu_device)
    outs = []
    for v in (0, 1):
        e = Engine(topo.variant, topo.input_nc, 1, topo.output_nc, topo.ngf, topo.num_downs, topo.size, max_batch=1, tune={"smallm_static": v})
        e.load_state_dict(sd)
        e.bind(e.pack(), gpu_device)
        shapes = {(l["h_in"], l["h_out"]) for l in e.layers(1) if l["kernel"] == "conv3x3_smallm"}
        assert {(4, 4), (4, 2), (2, 2), (2, 4)} <= shapes, shapes
        outs.append(e.forward(f, c).clone())
        e.close()
    assert torch.equal(outs[0], outs[1])
    assert np.abs(outs[1].cpu().numpy() - arrays["out"][:1]).max() <= 5e-5        # test_gpu_network.TIGHT
    with pytest.raises(N.Lspf2fError, match="smallm_static takes 0 .* or 1"):
        Engine(topo.variant, tune={"smallm_static": 2})
