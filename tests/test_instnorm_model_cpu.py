"""CPU: the bound tests/test_gpu_instnorm_layer.py holds the InstanceNorm kernels to -- |y - y64| <= 4 x the floor of fp32, per channel -- is
(a) attainable: the numpy restatement of the two standalone routes (tests/instnorm_model.py: the kernels' groupings, order and precisions) stays
inside it on every shape and input family the GPU test lists, and (b) has teeth: three deliberately wrong statistics each break it."""
import numpy as np
import pytest

import instnorm_model as M

FACTOR = 4.0
SMALL_HW = (4, 9, 31, 32, 33, 64, 65, 144, 256, 257, 576, 1024, 1025)
SMALL_C = (4, 32, 96, 160)
REDUCE_HW = (1, 63, 64, 65, 1296, 4097)
REDUCE_C = (4, 96, 160, 1024)


def worst_ratio(y, y64, mean64, var64):
    """max over the channels of max|y - y64| / floor, and the family of the channel that sets it"""
    ratio = np.abs(y.astype(np.float64) - y64).max(0) / M.floor32(y64, mean64, var64)
    return float(ratio.max()), int(ratio.argmax())


def problem(hw, c, offset, residual):
    rng = np.random.default_rng(1000 * hw + c + offset)
    x = M.make_input(rng, hw, c, offset)
    res = rng.standard_normal((hw, c)).astype(np.float32) if residual else None
    return x, res


def run(route, hw, c, **wrong):
    """every family lands on every channel position at C = 4 too: all seven offsets there, two elsewhere"""
    worst = (0.0, "")
    for offset in (range(7) if c == 4 else (0, 3)):
        x, res = problem(hw, c, offset, residual=offset % 2 == 1)
        y64, mean64, var64 = M.reference64(x, res, relu=offset % 3 == 2)
        y = route(x, res, offset % 3 == 2, **wrong)[0]
        r, ch = worst_ratio(y, y64, mean64, var64)
        worst = max(worst, (r, M.FAMILIES[M.family_of(ch, offset)]))
    return worst


@pytest.mark.parametrize("c", SMALL_C)
def test_small_route_model_stays_inside_the_bound(c):
    worst = max((run(M.small_route, hw, c) + (hw,)) for hw in SMALL_HW)
    print("\nin_small model, C %d: worst err / floor %.2f (%s, hw %d)" % ((c,) + worst))
    assert worst[0] <= FACTOR


@pytest.mark.parametrize("c", REDUCE_C)
def test_reduce_route_model_stays_inside_the_bound(c):
    worst = max((run(M.reduce_route, hw, c) + (hw,)) for hw in REDUCE_HW)
    print("\nreduce model, C %d: worst err / floor %.2f (%s, hw %d)" % ((c,) + worst))
    assert worst[0] <= FACTOR


@pytest.mark.parametrize("route,shapes", [(M.small_route, [(hw, c) for hw in SMALL_HW for c in SMALL_C]), (M.reduce_route, [(hw, c) for hw in REDUCE_HW for c in REDUCE_C])],
                         ids=["small", "reduce"])
def test_split_k_partials_stay_inside_the_bound(route, shapes):
    """splits = 3 with bias: the reference is the float64 sum of the slices, so the fold's own rounding counts against the bound"""
    worst = (0.0, None)
    for hw, c in shapes:
        for offset in (1, 4):
            rng = np.random.default_rng(77 * hw + c + offset)
            partial, bias, x64 = M.split_partials(rng, M.make_input(rng, hw, c, offset), 3)
            y64, mean64, var64 = M.reference64(x64)
            x, exact = M.fold(partial, bias, exact=True)
            y, mean, rstd = route(x, exact=exact) if route is M.reduce_route else route(x)
            r, ch = worst_ratio(y, y64, mean64, var64)
            if route is M.reduce_route:                    # what the GPU test asks of mean_out / rstd_out: the statistics of the slices' exact sum
                r64 = 1.0 / np.sqrt(var64 + M.EPS)
                assert (np.abs(mean - mean64) <= M.ulp32(mean64)).all(), (hw, c)
                assert (np.abs(rstd - r64) / r64 <= M.rstd_rel_bound(var64)).all(), (hw, c)
            worst = max(worst, (r, (hw, c, M.FAMILIES[M.family_of(ch, offset)])), key=lambda t: t[0])
    print("\nsplit-K partials through %s: worst err / floor %.2f %s" % (route.__name__, worst[0], worst[1]))
    assert worst[0] <= FACTOR


def test_model_statistics_meet_the_bounds_on_mean_and_rstd():
    """what the GPU test asks of mean_out / rstd_out, asked of the model of the route that produces them"""
    for hw in REDUCE_HW:
        for c in (4, 96):
            x, _ = problem(hw, c, 0, False)
            _, mean, rstd = M.reduce_route(x)
            _, mean64, var64 = M.reference64(x)
            assert (np.abs(mean - mean64) <= M.ulp32(mean64)).all(), (hw, c)
            r64 = 1.0 / np.sqrt(var64 + M.EPS)
            assert (np.abs(rstd - r64) / r64 <= M.rstd_rel_bound(var64)).all(), (hw, c)


def test_split_k_fold_rounds_once():
    """partials of size 1 that cancel to a flat 0.1: the folded tensor is within half an ulp OF 0.1, which an fp32 sum of the partials is not"""
    rng = np.random.default_rng(5)
    noise = rng.standard_normal((2, 65, 8)).astype(np.float32)
    p = np.concatenate([(np.float32(0.1) - noise.sum(0))[None], noise]).astype(np.float32)
    exact = p.astype(np.float64).sum(0)
    assert (np.abs(M.fold(p, None) - exact) <= 0.5 * M.ulp32(exact)).all()
    assert (np.abs(((p[0] + p[1]) + p[2]) - exact) > 2 * M.ulp32(exact)).any()


# ---- three wrong statistics kernels: each must be caught on at least one listed case -------------------------------------------------------------
def tail_counted_as_full(g, groups, hw, rows_per_group):
    return float(rows_per_group)


def merge_by_averaging_means(a, b):
    """groups combined as if their means and spreads were independent of each other: the mean of the group means, no between-group term"""
    if b[0] == 0:
        return a
    if a[0] == 0:
        return b
    n = a[0] + b[0]
    return n, (a[1] * a[0] + b[1] * b[0]) / n, a[2] + b[2]


def raw_moments_route(x, residual=None, relu=False):
    """var = E[x^2] - mean^2 from fp32 sums of the raw values (row order)"""
    s1 = np.zeros(x.shape[1], np.float32)
    s2 = np.zeros(x.shape[1], np.float32)
    for r in range(x.shape[0]):
        s1, s2 = s1 + x[r], s2 + x[r] * x[r]
    mean = (s1.astype(np.float64) / x.shape[0]).astype(np.float32)
    var = np.maximum(s2.astype(np.float64) / x.shape[0] - mean.astype(np.float64) ** 2, 0.0)
    rstd = (1.0 / np.sqrt(var + M.EPS)).astype(np.float32)
    return M.normalise(x, mean, rstd, residual, relu), mean, rstd


def test_a_tail_group_counted_as_64_rows_breaks_the_bound():
    assert run(M.reduce_route, 1296, 96)[0] <= FACTOR
    bad = max(run(M.reduce_route, hw, 96, count=tail_counted_as_full) for hw in (63, 65, 1296, 4097))
    print("\ntail counted as 64: err / floor %.3g (%s)" % bad)
    assert bad[0] > FACTOR
    assert run(M.reduce_route, 64, 96, count=tail_counted_as_full)[0] <= FACTOR      # no tail, no harm: the variant is wrong only where it should be


def test_variance_from_raw_moments_breaks_the_bound():
    bad_small = max(run(raw_moments_route, hw, 32) for hw in (256, 1024))
    bad_reduce = max(run(raw_moments_route, hw, 96) for hw in (1296, 4097))
    print("\nE[x^2] - mean^2: err / floor %.3g (%s) at the small route's shapes, %.3g (%s) at the reduce route's" % (bad_small + bad_reduce))
    assert bad_small[0] > FACTOR and bad_reduce[0] > FACTOR
    assert bad_small[1] != "normal" and bad_reduce[1] != "normal"                    # it is the |mean| >> std channels that give it away


def test_groups_merged_by_averaging_means_break_the_bound():
    bad = max(run(M.reduce_route, hw, 96, merge=merge_by_averaging_means) for hw in (65, 1296, 4097))
    print("\ngroup means averaged: err / floor %.3g (%s)" % bad)
    assert bad[0] > FACTOR
    assert run(M.reduce_route, 64, 96, merge=merge_by_averaging_means)[0] <= FACTOR  # one group: nothing to merge
