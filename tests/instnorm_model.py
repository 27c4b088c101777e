"""A numpy restatement of the arithmetic of the two standalone InstanceNorm routes (csrc/instnorm.hip): the same groupings in the same
order and the same precisions as the kernels, one frame [hw][C] at a time, vectorised over the channels.  Also what the CPU and the GPU
tests of those routes share: the float64 reference, the error floor of any fp32 InstanceNorm, and the input families.

Two places follow the compiler rather than the source text: in_small's `s2 += d * d` is contracted to one fused multiply-add by hipcc's default
-ffp-contract=fast, so the model forms d * d exactly (float64 holds the 48-bit product) and rounds the sum once -- through float64, which can
differ from a true fp32 fma in rare double-rounding cases; nothing here relies on bit equality with the device.  The normalisation is left
as written, (x - mean) * rstd, then + residual: a contraction there only removes a rounding."""
import numpy as np

EPS = 1e-5
F32 = np.float32


def fold(partial, bias, exact=False):
    """split-K partials [splits][hw][C] (+ bias [C]) -> the raw tensor, as fold_row adds them: ascending z in double, then the bias, rounded once;
    exact: also the float64 sum before that rounding, which in_reduce_stats takes its statistics from"""
    v = partial[0].astype(np.float64)
    for z in range(1, partial.shape[0]):
        v = v + partial[z]
    v = v + bias if bias is not None else v
    return (v.astype(F32), v) if exact else v.astype(F32)


def _fma_acc(acc, d):
    """acc + d * d with one rounding to fp32 (see the module docstring)"""
    return (acc.astype(np.float64) + d.astype(np.float64) * d.astype(np.float64)).astype(F32)


def normalise(x, mean, rstd, residual=None, relu=False):
    """normalise_v: fp32 throughout"""
    y = (x - mean[None, :].astype(F32)) * rstd[None, :].astype(F32)
    if residual is not None:
        y = y + residual.astype(F32)
    return np.maximum(y, F32(0)) if relu else y


# ---- in_small ------------------------------------------------------------------------------------------------------------------------------
def _block_sum(lanes):
    """lanes [32][C] (fp32, or float64 for the mean) -> float64 [C]: an xor tree in the lanes' own precision over the 8 row lanes of each wave (row lane bits
    0, 1, 2), then the 4 waves in order in double"""
    w = lanes.reshape(4, 8, -1)
    for o in (1, 2, 4):
        w = w + w[:, np.arange(8) ^ o, :]              # every lane adds its partner: commutative, so all lanes of a wave agree
    out = w[0, 0].astype(np.float64)
    for k in range(1, 4):
        out = out + w[k, 0].astype(np.float64)
    return out


def small_stats(x):
    """x [hw][C] fp32 -> (mean fp32 [C], rstd fp32 [C]) as in_small forms them: two passes, 32 row lanes striding the rows.  The sum behind the mean is carried
    in double from the first addition and rounded once; the squared deviations from that fp32 mean are summed in fp32 per lane and wave."""
    hw, c = x.shape
    steps = (hw + 31) // 32
    pad = np.zeros((steps * 32, c), F32)
    pad[:hw] = x
    rows = pad.reshape(steps, 32, c)                   # rows[i][rl] = row rl + 32 i
    live = (np.arange(steps * 32) < hw).reshape(steps, 32, 1)
    s1 = np.zeros((32, c), np.float64)
    for i in range(steps):
        s1 = np.where(live[i], s1 + rows[i], s1)
    mean = (_block_sum(s1) / hw).astype(F32)
    s2 = np.zeros((32, c), F32)
    for i in range(steps):
        s2 = np.where(live[i], _fma_acc(s2, rows[i] - mean[None, :]), s2)
    rstd = (1.0 / np.sqrt(_block_sum(s2) / hw + EPS)).astype(F32)
    return mean, rstd


def small_route(x, residual=None, relu=False):
    mean, rstd = small_stats(x)
    return normalise(x, mean, rstd, residual, relu), mean, rstd


# ---- in_reduce_stats -> in_finalize -> in_apply ------------------------------------------------------------------------------------------------
def group_sums(x, rows_per_group=64):
    """x [hw][C] (fp32; float64 for the exact sums of split-K slices) -> per group of 64 rows (s1, s2, shift) fp32 [G][C] as in_reduce_stats leaves them.
    256 / (C / 4) row lanes stride the group's rows and are added in lane order, twice: the sum of the values gives the shift c = the group's mean rounded to
    fp32, then the sums of d = x - c and d^2.  Everything is carried in double and rounded once, to the fp32 that in_finalize reads."""
    hw, c = x.shape
    g = (hw + rows_per_group - 1) // rows_per_group
    rl_n = min(256 // (c // 4), rows_per_group)        # lanes past the group's rows hold zeros: adding them changes nothing
    steps = (rows_per_group + rl_n - 1) // rl_n
    pad = np.zeros((g * rows_per_group, c), np.float64)
    pad[:hw] = x
    grp = pad.reshape(g, rows_per_group, c)
    live = (np.arange(g * rows_per_group) < hw).reshape(g, rows_per_group, 1)
    count = live.sum(1).astype(np.float64)             # [G][1]

    def lane_sums(values):
        acc = np.zeros((g, rl_n, c), np.float64)
        for k in range(steps):
            r = np.arange(rl_n) + k * rl_n
            ok = r < rows_per_group
            r = np.minimum(r, rows_per_group - 1)
            acc = np.where(live[:, r, :] & ok[None, :, None], acc + values[:, r, :], acc)
        total = acc[:, 0]
        for k in range(1, rl_n):
            total = total + acc[:, k]
        return total

    shift = (lane_sums(grp) / count).astype(F32)
    d = grp - shift[:, None, :]
    return lane_sums(d).astype(F32), lane_sums(d * d).astype(F32), shift


def group_moments(s1, s2, shift, n):
    """(count, mean, sum of squared deviations) of one group, in double"""
    m = s1.astype(np.float64) / n
    return n, shift.astype(np.float64) + m, s2.astype(np.float64) - s1.astype(np.float64) * m


def chan_merge(a, b):
    """the pairwise update of Chan, Golub & LeVeque; an empty side returns the other"""
    if b[0] == 0:
        return a
    if a[0] == 0:
        return b
    n = a[0] + b[0]
    delta = b[1] - a[1]
    return n, a[1] + delta * (b[0] / n), a[2] + b[2] + delta * delta * (a[0] * b[0] / n)


def true_count(g, groups, hw, rows_per_group):
    """rows behind group g: the last group of a frame may be short"""
    tail = hw - (hw // rows_per_group) * rows_per_group
    return float(tail) if tail and g == groups - 1 else float(rows_per_group)


def finalize(s1, s2, shift, hw, rows_per_group=64, count=true_count, merge=chan_merge):
    """in_finalize: lane l merges groups l, l + 64, ... in order, then an xor tree over the 64 lanes, lower lane first; everything in double.
    -> (mean fp32 [C], rstd fp32 [C]).  `count` and `merge` are parameters so that a test can put a wrong one in their place."""
    groups, c = s1.shape
    empty = (0.0, np.zeros(c), np.zeros(c))
    lanes = [empty] * 64
    for g in range(groups):
        lanes[g % 64] = merge(lanes[g % 64], group_moments(s1[g], s2[g], shift[g], count(g, groups, hw, rows_per_group)))
    while len(lanes) > 1:                              # lane 0's view of the tree: (0, 1), (2, 3), ... then pairs of pairs
        lanes = [merge(lanes[i], lanes[i + 1]) for i in range(0, len(lanes), 2)]
    n, mean, m2 = lanes[0]
    var = np.maximum(m2 / n, 0.0)
    return mean.astype(F32), (1.0 / np.sqrt(var + EPS)).astype(F32)


def reduce_route(x, residual=None, relu=False, count=true_count, merge=chan_merge, exact=None):
    """exact: the float64 sums of the split-K slices x was rounded from, if it was folded from any"""
    s1, s2, shift = group_sums(x if exact is None else exact)
    mean, rstd = finalize(s1, s2, shift, x.shape[0], 64, count, merge)
    return normalise(x, mean, rstd, residual, relu), mean, rstd


# ---- the float64 reference and the floor of fp32 ---------------------------------------------------------------------------------------------
def reference64(x, residual=None, relu=False):
    """x [hw][C] (any float type; split-K callers pass the float64 sum of partials + bias) -> (y, mean, biased var) in float64"""
    x = x.astype(np.float64)
    mean, var = x.mean(0), x.var(0)
    y = (x - mean) / np.sqrt(var + EPS)
    if residual is not None:
        y = y + residual.astype(np.float64)
    return (np.maximum(y, 0.0) if relu else y), mean, var


def ulp32(v):
    return np.spacing(np.abs(v).astype(F32)).astype(np.float64)


def floor32(y64, mean64, var64):
    """The best any fp32 InstanceNorm can do on a channel: the mean rounded to fp32 is off by up to half an ulp, which rstd amplifies; the subtraction, the
    product and the residual add each round once more.  [C]"""
    rstd = 1.0 / np.sqrt(var64 + EPS)
    return rstd * 0.5 * ulp32(mean64) + 2.0 ** -23 * (1.0 + np.abs(y64).max(0))


def rstd_rel_bound(var64):
    """relative error allowed on rstd: an fp32 sum of at most 64 non-negative squares per group (merged in double) perturbs var by 64 * 2^-24 relative, of which
    rstd = (var + eps)^-1/2 sees var / (var + eps) / 2 -- held to 4x that with the 1/2 dropped, plus the rounding of rstd itself to fp32"""
    return 4 * 64 * 2.0 ** -24 * var64 / (var64 + EPS) + 2.0 ** -23


# ---- input families --------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("normal", "mean1_std1e-2", "mean10_std1e-3", "mean-3_std1e-3", "constant", "constant_but_one_row", "ramp")


def family_of(c, offset=0):
    """neighbouring channels and neighbouring channel quads differ"""
    return (c + c // 4 + offset) % len(FAMILIES)


def make_input(rng, hw, c, offset=0):
    """[hw][c] fp32, family_of(channel) per channel"""
    x = np.empty((hw, c), np.float64)
    r = np.arange(hw, dtype=np.float64)
    for ch in range(c):
        f = family_of(ch, offset)
        if f == 0:
            x[:, ch] = rng.standard_normal(hw)
        elif f == 1:
            x[:, ch] = 1.0 + 1e-2 * rng.standard_normal(hw)
        elif f == 2:
            x[:, ch] = 10.0 + 1e-3 * rng.standard_normal(hw)
        elif f == 3:
            x[:, ch] = -3.0 + 1e-3 * rng.standard_normal(hw)
        elif f == 4:
            x[:, ch] = 0.1
        elif f == 5:
            x[:, ch] = 0.1
            x[int(rng.integers(hw)), ch] = 1.5
        else:
            x[:, ch] = 0.01 * r                         # group means differ strongly: a wrong merge shows
    return x.astype(F32)


def split_partials(rng, x, splits):
    """x [..., C] fp32 -> (partial [splits][..., C] fp32, bias [C] fp32, the float64 tensor they add up to): slices of size 1 that cancel to the family's tensor
    (to the rounding of the first slice), the way the K slices of a conv do"""
    bias = rng.standard_normal(x.shape[-1]).astype(F32)
    noise = (0.5 * rng.standard_normal((splits - 1,) + x.shape)).astype(F32)
    first = (x - bias) - noise.sum(0)
    partial = np.concatenate([first[None], noise]).astype(F32)
    return partial, bias, partial.astype(np.float64).sum(0) + bias.astype(np.float64)
