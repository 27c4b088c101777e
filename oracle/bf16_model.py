"""ORACLE (test infrastructure only) -- an exact numerical MODEL of the 16-bit storage paths (LSPF2F_DTYPE_BF16 and
LSPF2F_DTYPE_F16), for the whole network and layer by layer.

The reference has no bf16 path and only an autocast fp16 one (feature2face_G.py:28-30), so nothing of the reference can pin
these plans.  This file states precisely what the kernels are supposed to compute, so that the GPU path can be held to a
definite specification instead of a loose distance from the fp32 reference:

  * every activation tensor the kernels keep in the workspace is 16-bit -- bf16, or IEEE binary16 with its subnormals and
    its overflow to inf: each layer's epilogue result (acc * scale + shift, + residual, ReLU) is rounded to nearest-even
    once, on store;
  * conv weights of the implicit-GEMM layers are 16-bit (rounded once by the host packer); up-convs writing >= 32x32 and
    the last conv use the sub-pixel form -- the 3x3 taps that alias onto the same low-res pixel are summed in double,
    rounded to fp32, THEN to 16 bits (csrc/plan.cpp pack());
  * the first conv reads the fp32 API tensors with fp32 weights; the last conv returns fp32 (pre-tanh never rounded);
  * accumulation, BatchNorm scale/shift (folded in double, stored fp32), residual add, ReLU and tanh are fp32.
Accumulation ORDER is not part of the model: GPU and model differ by fp32 rounding before the 16-bit rounding, which now
and then flips a stored result by one unit in the last place.  Tests therefore look at the distribution of differences
(almost all zero, a thin tail of single-ulp flips with no sign preference), not only at the maximum.

Layer by layer (``layer_specs`` / ``layer_forward`` / ``LayerCheck``): the same arithmetic per named layer of the plan,
with the wiring -- source tensors in concat order, residual source, state-dict keys, stride, upsample, weight form --
derived from the reference network's nesting (the walk of oracle/torch_oracle.py), never from the plan, so that a wiring
mistake of csrc/plan.cpp shows up as a mismatch instead of being copied into the expectation."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

UP4_MIN_EXTENT = 32          # csrc/plan.h kUp4MinExtent

# (significand bits incl. the implicit one, smallest normal exponent, largest finite value)
FORMATS = {"bf16": (8, -126, 3.3895313892515355e38), "f16": (11, -14, 65504.0)}
TORCH_DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def rb(t: torch.Tensor) -> torch.Tensor:
    """round to nearest-even bf16, back to fp32"""
    return t.to(torch.bfloat16).to(torch.float32)


def round16(t: torch.Tensor, dtype: str) -> torch.Tensor:
    """Round to nearest-even in the 16-bit storage format, exactly, from fp32 or float64 (no double rounding through fp32);
    returns the input's dtype.  fp16 keeps its subnormals and overflows to +-inf."""
    if t.dtype == torch.float32:
        return t.to(TORCH_DTYPES[dtype]).to(torch.float32)
    p, emin, vmax = FORMATS[dtype]
    t = t.double()
    _, e = torch.frexp(t)                                   # t = m * 2**e, 0.5 <= |m| < 1
    q = torch.ldexp(torch.ones_like(t), torch.clamp(e - 1, min=emin) - (p - 1))
    r = torch.round(t / q) * q                              # t / q is exact; torch.round is half-to-even
    return torch.where(r.abs() > vmax, torch.copysign(torch.full_like(r, float("inf")), r), r)


def ulp16(v: torch.Tensor, dtype: str) -> torch.Tensor:
    """one unit in the last place of the 16-bit format at magnitude |v| (float64), with the format's subnormal floor"""
    p, emin, _ = FORMATS[dtype]
    _, e = torch.frexp(v.double())
    e = torch.where(v == 0, torch.full_like(e, emin + 1), e)
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), torch.clamp(e - 1, min=emin) - (p - 1))


def _affine(sd, key):
    g, b = sd[key + ".weight"].double(), sd[key + ".bias"].double()
    m, v = sd[key + ".running_mean"].double(), sd[key + ".running_var"].double()
    s = g / torch.sqrt(v + 1e-5)
    return s.float().view(1, -1, 1, 1), (b - m * s).float().view(1, -1, 1, 1)


def _fold(w: torch.Tensor) -> torch.Tensor:
    """[co][ci][3][3] -> [4 parities][co][ci][2][2]: pre-summed taps of Upsample(x2, nearest) + Conv3x3 (plan.cpp pack())."""
    lo = [[0, 1], [0, 2]]
    hi = [[0, 2], [1, 2]]
    wd = w.double()
    out = torch.zeros((4,) + tuple(w.shape[:2]) + (2, 2), dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    out[py * 2 + px, :, :, a, b] = wd[:, :, lo[py][a]:hi[py][a] + 1, lo[px][b]:hi[px][b] + 1].sum((2, 3))
    return out.float()


def _up_subpixel(x: torch.Tensor, wf: torch.Tensor) -> torch.Tensor:
    """out[2y+py, 2x+px] = sum_{a,b} wf[par][.., a, b] * x[y+py-1+a, x+px-1+b]  (zero outside)"""
    B, _, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.empty((B, wf.shape[1], 2 * H, 2 * W), dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], wf[py * 2 + px])
    return out


def generator_forward_16(sd: Dict[str, torch.Tensor], x: torch.Tensor, nres: int, num_downs: int = 8, dtype: str = "bf16",
                         prefix: str = "netG.model", pre_tanh: bool = False, rounding: bool = True) -> torch.Tensor:
    """The whole network under the storage model of ``dtype`` ("bf16" | "f16"); ``rounding=False`` keeps every value fp32
    (the same arithmetic with the 16-bit roundings switched off)."""
    rq = (lambda t: round16(t, dtype)) if rounding else (lambda t: t)

    def conv(h, key, stride=1):                       # implicit-GEMM layer: 16-bit weights, 16-bit inputs, fp32 accumulate
        return F.conv2d(h, rq(sd[key]), None, stride, 1)

    def res(h, key):
        s1, t1 = _affine(sd, key + ".block.1")
        s2, t2 = _affine(sd, key + ".block.4")
        a = rq(F.relu(conv(h, key + ".block.0.weight") * s1 + t1))
        return rq(F.relu(conv(a, key + ".block.3.weight") * s2 + t2 + h))

    def level(xin, pfx, depth):
        outer, inner = depth == 0, depth == num_downs - 1
        i = 0
        wkey = "%s.model.%d.weight" % (pfx, i)
        if outer:
            h = F.conv2d(xin, sd[wkey], None, 2, 1)               # first conv: fp32 inputs and weights
        else:
            h = conv(xin, wkey, 2)
        i += 1
        if not (outer or inner):
            s, t = _affine(sd, "%s.model.%d" % (pfx, i))
            h = h * s + t
            i += 1
        h = rq(F.relu(h))
        i += 1
        for _ in range(nres):
            h = res(h, "%s.model.%d" % (pfx, i))
            i += 1
        if not inner:
            h = level(h, "%s.model.%d" % (pfx, i), depth + 1)
            i += 1
        i += 1                                                     # Upsample
        w = sd["%s.model.%d.weight" % (pfx, i)]
        ho = 2 * h.shape[-1]
        if outer or ho >= UP4_MIN_EXTENT:
            y = _up_subpixel(h, rq(_fold(w)))                      # sub-pixel form, folded taps rounded to 16 bits
        else:
            y = F.conv2d(F.interpolate(h, scale_factor=2, mode="nearest"), rq(w), None, 1, 1)
        i += 1
        if outer:
            return y                                               # fp32, never rounded
        s, t = _affine(sd, "%s.model.%d" % (pfx, i))
        y = rq(F.relu(y * s + t))
        i += 2
        for _ in range(nres):
            y = res(y, "%s.model.%d" % (pfx, i))
            i += 1
        return torch.cat([xin, y], 1)

    with torch.no_grad():
        y = level(x.float(), prefix, 0)
        return y if pre_tanh else torch.tanh(y)


def generator_forward_bf16(sd: Dict[str, torch.Tensor], x: torch.Tensor, nres: int, num_downs: int = 8,
                           prefix: str = "netG.model", pre_tanh: bool = False) -> torch.Tensor:
    return generator_forward_16(sd, x, nres, num_downs, "bf16", prefix, pre_tanh)


# ---- the per-layer decomposition ---------------------------------------------------------------------------------------

INPUT = "input"              # the API tensor cat([feature_map, cand_image], 1) the first conv reads (fp32)


@dataclass(frozen=True)
class LayerSpec:
    """One stored layer of a 16-bit plan, named as the planner names it."""
    name: str                 # L{d}.down, L{d}.d.res{i}.a / .b, L{d}.up, L{d}.u.res{i}.a / .b
    kind: str                 # "first" (fp32 operands) | "conv" (16-bit, stride 1 or 2) | "up9" (nearest x2 + 9 taps) | "up4" (sub-pixel) | "last"
    srcs: Tuple[str, ...]     # producing layers of the input tensors, in concat order (INPUT for the API tensor)
    res: Optional[str]        # producing layer of the residual (second conv of a ResidualBlock), else None
    wkey: str                 # state-dict key of the OIHW weight
    bnkey: Optional[str]      # state-dict prefix of the BatchNorm2d folded into the epilogue, else None
    stride: int
    upsample: bool
    form: str                 # weight form the layer reads: "fp32" (first conv), "rows" (9 taps) or "up4" (folded sub-pixel taps)
    cin: int
    cout: int
    h_in: int                 # extent of the tensor(s) read (pre-upsample)
    h_out: int


def _level_channels(depth: int, ngf: int, input_nc: int, output_nc: int) -> Tuple[int, int, int]:
    """networks.py:557-570: (down-conv input, inner, up-conv output) channels of nesting depth ``depth``"""
    if depth == 0:
        return input_nc, ngf, output_nc
    return ngf * min(2 ** (depth - 1), 8), ngf * min(2 ** depth, 8), ngf * min(2 ** (depth - 1), 8)


def layer_specs(nres: int, num_downs: int = 8, size: int = 512, ngf: int = 64, input_nc: int = 13, output_nc: int = 3,
                prefix: str = "netG.model") -> List[LayerSpec]:
    """Every conv of the generator in execution order, walked over the reference's nesting exactly like
    torch_oracle.generator_forward walks it (same Sequential indices, same skip / concat structure)."""
    out: List[LayerSpec] = []

    def res_blocks(L: str, side: str, pfx: str, i: int, x: str, c: int, h: int) -> Tuple[int, str]:
        for r in range(nres):
            key = "%s.model.%d" % (pfx, i)
            a = "%s.%s.res%d.a" % (L, side, r)
            b = "%s.%s.res%d.b" % (L, side, r)
            out.append(LayerSpec(a, "conv", (x,), None, key + ".block.0.weight", key + ".block.1", 1, False, "rows", c, c, h, h))
            out.append(LayerSpec(b, "conv", (a,), x, key + ".block.3.weight", key + ".block.4", 1, False, "rows", c, c, h, h))
            x = b
            i += 1
        return i, x

    def level(pfx: str, depth: int, x: str, h_in: int) -> str:
        outer, inner = depth == 0, depth == num_downs - 1
        cin, mid, cout = _level_channels(depth, ngf, input_nc, output_nc)
        L, h = "L%d" % depth, h_in // 2
        i = 0
        wkey = "%s.model.%d.weight" % (pfx, i)
        i += 1
        bn = None
        if not (outer or inner):
            bn = "%s.model.%d" % (pfx, i)
            i += 1
        out.append(LayerSpec(L + ".down", "first" if outer else "conv", (x,), None, wkey, bn, 2, False,
                             "fp32" if outer else "rows", cin, mid, h_in, h))
        i += 1                                                     # ReLU
        i, cur = res_blocks(L, "d", pfx, i, L + ".down", mid, h)
        srcs: Tuple[str, ...] = (cur,)
        if not inner:
            srcs = (cur, level("%s.model.%d" % (pfx, i), depth + 1, cur, h))      # cat([x, model(x)], 1) of the level below
            i += 1
        i += 1                                                     # Upsample
        wkey = "%s.model.%d.weight" % (pfx, i)
        i += 1
        up4 = outer or h_in >= UP4_MIN_EXTENT
        if outer:
            out.append(LayerSpec(L + ".up", "last", srcs, None, wkey, None, 1, True, "up4", mid * len(srcs), cout, h, h_in))
            return ""
        out.append(LayerSpec(L + ".up", "up4" if up4 else "up9", srcs, None, wkey, "%s.model.%d" % (pfx, i), 1, True,
                             "up4" if up4 else "rows", mid * len(srcs), cout, h, h_in))
        i += 2                                                     # BN, ReLU
        _, cur = res_blocks(L, "u", pfx, i, L + ".up", cout, h_in)
        return cur

    level(prefix, 0, INPUT, size)
    return out


# The kernels (lspf2f_layer_info_get names) whose arithmetic the model states, per kind of layer: every one reads the weight
# form of its kind (first conv: fp32 rows; 16-bit rows; 16-bit folded sub-pixel taps) and rounds once on store.  The direct
# last-conv kernel ("last_conv", tune key lastconv_direct) reads fp32 taps and is not covered.
_IGEMM = ("igemm3x3", "igemm3x3+splitk_reduce", "igemm3x3 (split-K combined in the launch)")
COVERED_KERNELS = {
    "first": ("first_conv",),
    "conv": _IGEMM + ("conv3x3_smallm", "conv3x3_fullk16", "conv3x3_patch16", "bandconv512", "rowconv64", "rowconv128"),
    "up9": _IGEMM + ("conv3x3_smallm", "conv3x3_fullk16"),
    "up4": _IGEMM + ("conv3x3_patchup16", "rowup256"),
    "last": ("last_conv (rowlast128 + pixel_shuffle_tanh)", "last_conv (igemm3x3 + pixel_shuffle_tanh)"),
}

# The 16-bit plans the layer-by-layer GPU test pins (variant, dtype, batch, frame size): the bench's timed plan (BASELINE
# configs[2]), its fp16 twin, the two-res-block variant, the batch-1 split-K / smallm route, the 3-frame plan that uses every
# 16-bit kernel, and another frame size
CHECKED_PLANS = [("normal", "bf16", 8, 512), ("normal", "f16", 8, 512), ("large", "bf16", 8, 512), ("large", "f16", 8, 512),
                 ("normal", "bf16", 1, 512), ("normal", "f16", 3, 512), ("normal", "bf16", 1, 1024)]


def layer_weight(spec: LayerSpec, sd: Dict[str, torch.Tensor], dtype: str, rounding: bool = True) -> torch.Tensor:
    """the weights exactly as the packer hands them to the layer's kernel (fp32 values): OIHW, or [4][co][ci][2][2] folded"""
    w = sd[spec.wkey].float()
    if spec.form == "fp32":
        return w
    if spec.form == "up4":
        w = _fold(w)
    return round16(w, dtype) if rounding else w


def layer_affine(spec: LayerSpec, sd: Dict[str, torch.Tensor]):
    """fp32 (scale, shift) of the epilogue, folded in double like plan.cpp pack(); (None, None) without BatchNorm"""
    return _affine(sd, spec.bnkey) if spec.bnkey else (None, None)


def _conv(spec: LayerSpec, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    if spec.form == "up4":
        return _up_subpixel(x, w)
    if spec.upsample:
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, None, 1, 1)
    return F.conv2d(x, w, None, spec.stride, 1)


def layer_forward(spec: LayerSpec, sd: Dict[str, torch.Tensor], srcs: Sequence[torch.Tensor], res: Optional[torch.Tensor],
                  dtype: str, rounding: bool = True) -> torch.Tensor:
    """The layer's stored result under the model, in fp32 arithmetic (the same operations, in the same order, as
    generator_forward_16); the last conv returns its fp32 pre-tanh output."""
    x = srcs[0] if len(srcs) == 1 else torch.cat(list(srcs), 1)
    y = _conv(spec, x, layer_weight(spec, sd, dtype, rounding))
    if spec.kind == "last":
        return y
    s, t = layer_affine(spec, sd)
    if s is not None:
        y = y * s + t
    if res is not None:
        y = y + res
    y = F.relu(y)
    return round16(y, dtype) if rounding else y


def forward_by_layers(specs: Sequence[LayerSpec], sd: Dict[str, torch.Tensor], x: torch.Tensor, dtype: str,
                      rounding: bool = True) -> Dict[str, torch.Tensor]:
    """every layer fed its own predecessors' outputs: name -> tensor (the last conv: pre-tanh)"""
    t: Dict[str, torch.Tensor] = {INPUT: x.float()}
    with torch.no_grad():
        for s in specs:
            t[s.name] = layer_forward(s, sd, [t[n] for n in s.srcs], t[s.res] if s.res else None, dtype, rounding)
    return t


# ---- the comparison ----------------------------------------------------------------------------------------------------

# fp32-accumulation allowance of the hard bound |g - y| <= ulp16(max(|g|, |y|)) + C_ACC * E, E = A + |shift| + |residual|,
# A = |s| (|Wq| conv |X|).  The GPU rounds an fp32 value ŷ to 16 bits; ŷ differs from the exact y by the fp32 rounding of
# the K-term sum and of the epilogue, which no ordering argument bounds below ~K * 2**-24 * A in the worst case but which
# a well-conditioned MFMA/FMA accumulation keeps near sqrt(K) * 2**-24 * A: the kernel guide measures an fp32 FMA chain at
# 3.5e-7 * sum|a*b| for K = 4096 (the largest K here is 9 * 1024 = 9216 taps x channels of a concat up-conv).  2**-19
# (1.9e-6) is ~5x that figure, and the GPU test measures what the 16-bit MFMAs actually need (`acc_ratio`: the largest
# excess of |g - y| over half an ulp, per unit of E -- a lower bound of the accumulation error) and prints the headroom.
# The allowance only matters where the sum nearly cancels: for a typical element |y| ~ A / sqrt(K) and one ulp is
# 2**-8 (bf16) / 2**-11 (fp16) of that, 4..30x more than C_ACC * A at K = 4608.
C_ACC = 2.0 ** -19
# fp32 bound of the last conv (fp32 output after tanh, never rounded): the accumulation allowance plus 4 fp32 ulps of
# tanhf, with the batch-1 test's absolute 2e-5 as a ceiling (test_gpu_network.py)
LAST_ABS = 2e-5

# Rounding statistics over the elements where the stored value or the rounded model is non-zero.  `flip` = fraction with
# g != round16(y); `chan_flip` = the largest such fraction of one output channel (over >= MIN_CHAN_ELEMS elements);
# `mean` = signed mean of (g - round16(y)) / ulp over the flips, each term clipped to [-1, 1] (near-cancelling sums differ by
# many ulps of their tiny result within the accumulation allowance and would otherwise decide the mean): truncating stores
# give -1 on ReLU outputs, a biased epilogue a biased tail.  It must stay within MEAN_BIAS + 3 / sqrt(flips).
# Measured on the shipped plans (tests/test_gpu_storage16_layers.py, every layer of bf16_model.CHECKED_PLANS): largest flip
# fraction 4e-4 (bf16) / 2.3e-3 (fp16, L3.d.res0.a at K = 4608: ~6x bf16's), largest per-channel fraction 0.012 / 0.058.
# The bars leave 5x / 4x (flip) and 3.4x / 2.6x (channel) of margin and stay far below what the planted faults of
# tests/test_storage16_model_cpu.py produce (truncation 0.5; double rounding 0.2 and more; one channel's scale 1e-3 off:
# 0.15-0.2 of that channel in bf16, 0.8-0.9 in fp16).
BARS = {
    "bf16": {"flip": 0.002, "chan_flip": 0.04},
    "f16": {"flip": 0.01, "chan_flip": 0.15},
}
MEAN_BIAS = 0.1
MIN_CHAN_ELEMS = 512
MIN_FLIPS = 50


class LayerCheck:
    """Accumulates, over the frames checked, how one layer's stored output g compares with the float64 model y computed
    from the GPU's own stored inputs; ``failures()`` lists what breaks the hard bound or a bar."""

    def __init__(self, spec: LayerSpec, dtype: str):
        self.spec, self.dtype = spec, dtype
        self.n = self.nz = self.flips = self.hard = 0
        self.sum_signed = 0.0
        self.worst_ulps = 0.0          # max |g - y| / ulp16(max(|g|, |y|))
        self.acc_ratio = 0.0           # max (|g - y| - ulp/2) / E: what the accumulation had to be allowed
        self.last_err = 0.0            # last conv: max |g - tanh(y)|
        self.chan_n = np.zeros(spec.cout, np.int64)
        self.chan_flips = np.zeros(spec.cout, np.int64)
        self.first_bad = ""

    def model(self, sd, srcs: Sequence[torch.Tensor], res: Optional[torch.Tensor]):
        """(y float64, E float64) for NCHW fp32 inputs holding the stored (16-bit or fp32 API) values"""
        spec = self.spec
        x = srcs[0] if len(srcs) == 1 else torch.cat(list(srcs), 1)
        w = layer_weight(spec, sd, self.dtype)
        y = _conv(spec, x.double(), w.double())
        e = _conv(spec, x.abs().float(), w.abs()).double()                     # no cancellation: fp32 is plenty
        if spec.kind == "last":
            return y, e
        s, t = layer_affine(spec, sd)
        if s is not None:
            y = y * s.double() + t.double()
            e = e * s.double().abs() + t.double().abs()
        if res is not None:
            y = y + res.double()
            e = e + res.double().abs()
        return torch.relu(y), e

    def add(self, g: torch.Tensor, y: torch.Tensor, e: torch.Tensor) -> None:
        """g: the stored output (NCHW, fp32 values); y, e from model()"""
        g = g.double()
        if self.spec.kind == "last":
            want = torch.tanh(y)
            d = (g - want).abs()
            lim = C_ACC * e + 4 * 2.0 ** -24 * torch.maximum(g.abs(), want.abs()) + 2.0 ** -40
            self.last_err = max(self.last_err, float(d.max()))
            bad = (d > lim) | (d > LAST_ABS)
            self._bad(bad, d)
            self.n += g.numel()
            return
        u = ulp16(torch.maximum(g.abs(), y.abs()), self.dtype)
        d = (g - y).abs()
        bad = d > u + C_ACC * e
        self._bad(bad, d / u)
        self.worst_ulps = max(self.worst_ulps, float((d / u).max()))
        self.acc_ratio = max(self.acc_ratio, float(((d - 0.5 * u) / e.clamp(min=1e-300)).max()))
        r = round16(y, self.dtype)
        nz = (g != 0) | (r != 0)
        flip = (g != r) & nz
        self.n += g.numel()
        self.nz += int(nz.sum())
        self.flips += int(flip.sum())
        if bool(flip.any()):
            self.sum_signed += float(((g - r)[flip] / ulp16(torch.maximum(g.abs(), r.abs())[flip], self.dtype)).clamp(-1, 1).sum())
        self.chan_n += nz.sum((0, 2, 3)).numpy()
        self.chan_flips += flip.sum((0, 2, 3)).numpy()

    def _bad(self, bad: torch.Tensor, what: torch.Tensor) -> None:
        nb = int(bad.sum())
        if nb and not self.first_bad:
            idx = tuple(int(v) for v in torch.nonzero(bad)[0])
            self.first_bad = "first at [frame-local n, c, y, x] = %s: %.4g" % (idx, float(what[idx]))
        self.hard += nb

    # ---- summaries
    @property
    def flip(self) -> float:
        return self.flips / max(self.nz, 1)

    @property
    def mean(self) -> float:
        return self.sum_signed / self.flips if self.flips else 0.0

    @property
    def chan_flip(self) -> float:
        ok = self.chan_n >= MIN_CHAN_ELEMS
        return float((self.chan_flips[ok] / self.chan_n[ok]).max()) if ok.any() else 0.0

    def failures(self) -> List[str]:
        f = []
        if self.hard:
            f.append("%d elements outside the hard bound (%s)" % (self.hard, self.first_bad))
        if self.spec.kind == "last":
            return f
        b = BARS[self.dtype]
        if self.flip > b["flip"]:
            f.append("flip fraction %.4f > %.3f" % (self.flip, b["flip"]))
        if self.chan_flip > b["chan_flip"]:
            f.append("per-channel flip fraction %.4f > %.3f" % (self.chan_flip, b["chan_flip"]))
        if self.flips >= MIN_FLIPS and abs(self.mean) > MEAN_BIAS + 3 / self.flips ** 0.5:
            f.append("signed mean of the flips %+.3f ulp over %d flips, |.| > %.3f" % (self.mean, self.flips, MEAN_BIAS + 3 / self.flips ** 0.5))
        return f

    def row(self, kernel: str = "") -> str:
        s = self.spec
        k = s.cin * 9 if s.form != "up4" else s.cin * 4
        if s.kind == "last":
            return "%-13s %-44s K %5d  max |g-tanh(y)| %.2e (fp32 output)" % (s.name, kernel, k, self.last_err)
        return "%-13s %-44s K %5d  worst %7.3f ulp  flips %.5f (chan %.4f)  mean %+.3f of %6d  acc %.2e" % (
            s.name, kernel, k, self.worst_ulps, self.flip, self.chan_flip, self.mean, self.flips, self.acc_ratio)
