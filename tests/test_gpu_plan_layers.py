"""A plan's layers against the per-layer entry point.  run_layer (a forward) and lspf2f_conv3x3 fill a kernel's arguments with the same builders, so
a layer of a plan, given again to lspf2f_conv3x3 -- its own inputs, its own packed weights, scale and shift, and the tile code that names its route -- must
write the bits the forward left in the workspace.  (The forward's Winograd launches carry `out_wt` and `wino_prio`, the per-layer call does not: both knobs are
bit-identical by construction, so there is no tolerance.)

The plans: the smallest fp32 plan whose layer table shows conv3x3_smallm, conv3x3_fullk, wino3x3<1>, winoup3x3<1> and an unsplit igemm3x3 -- found from the
layer tables of both variants x ngf 32 | 64 x 4..8 levels x 32..512 pixels x 1 | 2 frames: none below 512 pixels has all five -- and the smallest 16-bit plan with
conv3x3_patch16, a rowconv and conv3x3_fullk16 (likewise, 1..8 frames)."""
import ctypes

import pytest
import torch

from oracle import bf16_model as M

pytestmark = pytest.mark.gpu

# variant, ngf, num_downs, size, batch, dtype, the kernels one layer each is replayed for
PLANS = [
    ("normal", 32, 8, 512, 2, "f32", ("conv3x3_smallm", "conv3x3_fullk", "wino3x3<1>", "winoup3x3<1>", "igemm3x3")),
    ("normal", 64, 6, 512, 3, "bf16", ("conv3x3_patch16", "rowconv", "conv3x3_fullk16")),
]


def tile_code(l, spec, kernel):
    """(tile_m, tile_n, split_k, k_group, weight form) that name the route of layer-table row `l` to lspf2f_conv3x3"""
    two_sources = len(spec.srcs) == 2
    if kernel == "conv3x3_smallm":
        return 1, 1, 0, 0, "rows"
    if kernel == "conv3x3_fullk":          # K halves of a single source, and the stride-2 form, read the half-source packing
        return l["tile_m"], 16, l["split_k"], -1, "fullk2" if l["stride"] == 2 or (l["split_k"] == 2 and not two_sources) else "fullk"
    if kernel == "wino3x3<1>":             # 4003: one channel block per wave, U fragments in registers -- the form the plans take
        return 4003, 0, l["split_k"], -1, "wino"
    if kernel == "winoup3x3<1>":
        return 5001, 0, l["split_k"], -1, "winoup"
    if kernel == "igemm3x3":
        return l["tile_m"], l["tile_n"], l["split_k"], l["k_group"], "rows"
    if kernel == "conv3x3_patch16":        # 7000 + tile width (64 at 64x64, 32 at 32x32); tile_n = channels per workgroup, 64 = the deep-ring form the plans take
        return 7000 + (64 if l["h_out"] == 64 else 32), l["tile_n"], 0, 0, "rows"
    if kernel.startswith("rowconv"):       # 1000 + output rows per strip: a tile is (64 | 32) x R pixels of 64 | 128 channels
        return 1000 + l["tile_m"] // (64 if l["cin"] == 64 else 32), l["cin"], 0, -1, "row"
    if kernel == "conv3x3_fullk16":
        return l["tile_m"], 16, 0, -1, "fullk"
    raise KeyError(kernel)


@pytest.mark.parametrize("variant,ngf,num_downs,size,batch,dtype,kernels", PLANS, ids=[p[5] for p in PLANS])
def test_plan_layers_equal_the_per_layer_entry_point(variant, ngf, num_downs, size, batch, dtype, kernels, gpu_device):
    from livespeechportraits_amd import _native as N
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.engine import Engine
    from livespeechportraits_amd.topology import build_topology
    topo = build_topology(variant, ngf=ngf, num_downs=num_downs, size=size)
    e = Engine(variant, 13, 1, 3, ngf, num_downs, size, max_batch=batch, dtype=dtype, keep_intermediates=True)
    e.load_state_dict(synth.make_state_dict(topo, 1234))
    blob = e.pack().to(gpu_device)
    e.bind(blob)
    feat, cand = synth.make_inputs(batch, size, seed=99, cand_batch=1)
    e.forward(torch.from_numpy(feat).to(gpu_device), torch.from_numpy(cand).to(gpu_device))
    torch.cuda.synchronize()
    layers = e.layers(batch)
    specs = M.layer_specs(topo.nres, num_downs, size, ngf, topo.input_nc, topo.output_nc)      # the wiring: sources in concat order, residual
    assert [l["name"] for l in layers] == [s.name for s in specs]
    lib, dt = e.lib, N.DTYPE_IDS[dtype]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    in_blob = lambda off: ctypes.c_void_p(blob.data_ptr() + off) if off >= 0 else None
    for kernel in kernels:
        hits = [i for i, l in enumerate(layers) if (l["kernel"].startswith(kernel) if kernel == "rowconv" else l["kernel"] == kernel)]
        assert hits, "the plan has no %s layer (kernels: %s)" % (kernel, sorted({l["kernel"] for l in layers}))
        i = hits[0]
        l, s = layers[i], specs[i]
        tile_m, tile_n, split_k, k_group, form = tile_code(l, s, l["kernel"] if kernel == "rowconv" else kernel)
        srcs = [e.intermediate(n, batch) for n in s.srcs]
        res = e.intermediate(s.res, batch) if s.res else None
        want = e.intermediate(s.name, batch)
        c0, c1 = srcs[0].shape[3], srcs[1].shape[3] if len(srcs) == 2 else 0
        up = {"up4": 2, "up9": 1}.get(s.kind, 0)
        assert e.form_offset(i, form) >= 0, (s.name, form)
        shape = (batch, l["h_in"], l["h_in"], c0, c1, l["cout"], l["stride"], up)
        sb = lib.lspf2f_conv3x3_scratch_bytes(*shape, tile_m, tile_n, split_k, k_group, dt)
        scratch = torch.zeros(max(sb, 4), dtype=torch.uint8, device=gpu_device)          # (arrival counters start at zero)
        out = torch.full_like(want, float("nan"))
        N.check(lib.lspf2f_conv3x3(ptr(srcs[0]), ptr(srcs[1]) if c1 else None, in_blob(e.form_offset(i, form)), in_blob(l["scale_offset"]), in_blob(l["shift_offset"]),
                                   ptr(res), ptr(out), *shape, int(l["relu"]), tile_m, tile_n, split_k, k_group, dt, ptr(scratch), scratch.numel(),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        differ = int((out.view(torch.int16 if dt else torch.int32) != want.view(torch.int16 if dt else torch.int32)).sum())
        print("%s %s: layer %s on %s as tile %d x %d, split_k %d, k_group %d: %d of %d elements differ" % (
            variant, dtype, s.name, l["kernel"], tile_m, tile_n, split_k, k_group, differ, want.numel()))
        assert differ == 0, (s.name, l["kernel"])
    e.close()
