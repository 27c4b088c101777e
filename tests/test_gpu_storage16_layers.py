"""Every layer of the shipped 16-bit plans, fed its own inputs, against the exact storage model of oracle/bf16_model.py.

For each plan of bf16_model.CHECKED_PLANS: one forward with bench.py's weights and inputs (synth seed 1234, inputs seed 99,
shared candidates) on an engine that keeps every intermediate; then, frame by frame on the host, every layer's stored output is
compared with the float64 result of the model applied to the GPU's OWN stored inputs of that layer (the wiring -- sources in
concat order, residual, weight form -- comes from the reference network's nesting, not from the plan).  Hard bound per element:
|g - y| <= ulp16(max(|g|, |y|)) + C_ACC * E; per layer: flip fraction, per-channel flip fraction and signed mean of the flips
against the bars of bf16_model.BARS.  A layer on a kernel the model does not state fails.  The last conv: fp32 frames after
tanh.  Then the production engine (arena reuse on) must plan the same kernels and compute the same bits, and at 8 frames of
`normal` its uint8 frames must be tensor2im of its fp32 frames."""
import os
import time

import numpy as np
import pytest
import torch

from oracle import bf16_model as M

pytestmark = pytest.mark.gpu

# frames checked in full per batch: all of them for `normal`; 0, 1 and the last for `large` at 8 frames (1.5x the work per frame)
def _frames(variant, batch):
    return (0, 1, batch - 1) if variant == "large" and batch > 3 else tuple(range(batch))


def _engine(variant, dtype, batch, size, sd, dev, keep):
    from livespeechportraits_amd.engine import Engine
    e = Engine(variant, size=size, max_batch=batch, dtype=dtype, keep_intermediates=keep)
    e.load_state_dict(sd)
    e.bind(e.pack(), dev)
    return e


@pytest.mark.parametrize("variant,dtype,batch,size", M.CHECKED_PLANS)
def test_every_layer_of_the_16bit_plan_matches_the_storage_model(variant, dtype, batch, size, gpu_device):
    from livespeechportraits_amd import synth
    from livespeechportraits_amd.topology import build_topology
    from oracle import torch_oracle
    from oracle.tensor2im_oracle import tensor2im
    t_start = time.time()
    threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16")), threads)))   # a GPU box grants 16 CPUs
    try:
        topo = build_topology(variant, size=size)
        sd = synth.make_state_dict(topo, 1234)
        sdt = torch_oracle.to_torch(sd)
        feat, cand = synth.make_inputs(batch, size, seed=99, cand_batch=1)
        f, c = torch.from_numpy(feat).to(gpu_device), torch.from_numpy(cand).to(gpu_device)
        e = _engine(variant, dtype, batch, size, sd, gpu_device, keep=True)
        out = e.forward(f, c)
        torch.cuda.synchronize()
        layers = e.layers(batch)
        specs = M.layer_specs(topo.nres, topo.num_downs, size, topo.ngf, topo.input_nc, topo.output_nc)
        assert [l["name"] for l in layers] == [s.name for s in specs], "plan and model name different layers"
        uncovered = [(s.name, l["kernel"]) for l, s in zip(layers, specs) if l["kernel"] not in M.COVERED_KERNELS[s.kind]]
        assert not uncovered, "layers on kernels the storage model does not state: %s" % uncovered

        # the production engine (activation arena reused) plans the same kernels and computes the same bits
        p = _engine(variant, dtype, batch, size, sd, gpu_device, keep=False)
        key = lambda L: [(l["name"], l["kernel"], l["tile_m"], l["tile_n"], l["split_k"], l["k_group"]) for l in L]
        assert key(p.layers(batch)) == key(layers)
        out_p = p.forward(f, c)
        assert torch.equal(out_p, out), "keep_intermediates=False computes other bits"
        if batch == 8 and variant == "normal":
            # uint8 frames (two-launch last conv: rowlast128 + pixel_shuffle_tanh) against the fused fp32 forward and tensor2im
            u8, fl = p.forward_image(f, c, also_float=True)
            assert torch.equal(fl, out_p), "forward_image's fp32 frames != forward()'s"
            want = np.stack([tensor2im(v) for v in fl.cpu().numpy()])
            assert np.array_equal(u8.cpu().numpy(), want), "uint8 frames != tensor2im of the fp32 frames"
            assert torch.equal(p.forward_image(f, c), u8), "uint8-only call gives other bytes"
        out = out.cpu()
        t_gpu = time.time() - t_start

        x = torch.cat([torch.from_numpy(feat), torch.from_numpy(cand).expand(batch, -1, -1, -1)], 1)
        stored = {s.name: e.intermediate(s.name, batch) for s in specs if s.kind != "last"}
        checks = {s.name: M.LayerCheck(s, dtype) for s in specs}
        frames = _frames(variant, batch)
        for i in frames:
            cache = {M.INPUT: x[i:i + 1]}

            def get(name):
                if name not in cache:
                    cache[name] = stored[name][i:i + 1].cpu().float().permute(0, 3, 1, 2).contiguous()
                return cache[name]
            for s in specs:
                y, a = checks[s.name].model(sdt, [get(n) for n in s.srcs], get(s.res) if s.res else None)
                checks[s.name].add(out[i:i + 1] if s.kind == "last" else get(s.name), y, a)
        print("\n%s %s batch %d at %d^2: frames %s checked in full (%.0f s GPU + setup, %.0f s total)" % (
            variant, dtype, batch, size, list(frames), t_gpu, time.time() - t_start))
        for l, s in zip(layers, specs):
            print("  " + checks[s.name].row(l["kernel"]))
        acc = max(ch.acc_ratio for ch in checks.values() if ch.spec.kind != "last")
        print("  accumulation: largest (|g-y| - ulp/2) / E = %.3g; allowance C_ACC = %.3g (headroom %.1fx)" % (acc, M.C_ACC, M.C_ACC / max(acc, 1e-30)))
        bad = ["%s (%s): %s" % (s.name, l["kernel"], "; ".join(checks[s.name].failures())) for l, s in zip(layers, specs) if checks[s.name].failures()]
        assert not bad, "layers outside the storage model:\n" + "\n".join(bad)
    finally:
        torch.set_num_threads(threads)
