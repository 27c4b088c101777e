"""lspf2f_conv3x3_scratch_bytes is pure host arithmetic over the tile codes of lspf2f_conv3x3 (include/lspf2f.h): its answers were recorded from the
library before the codes were decoded in one place and the split-K layouts stated once, and must not move.

tests/golden/conv3x3_scratch_bytes.json holds arguments and results only.  The grid: every tile code x split_k {0, 1, 2, 4} x k_group {0, 1, -1, -4} x
dtype {0, 1} x three shapes the code's kernel family supports.  Each code comes with the tile_n its callers pass (0 for the Winograd codes, 128 | 64 | 65 for the
patch-staged ones).  Above 3000, tile_n 64 with k_group -1 is the up-conv row kernel's 3000 + R whatever tile_m says: the grid has that once, as 3008 x 64, and
leaves k_group -1 out for the patch-staged codes at tile_n 64."""
import itertools
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv3x3_scratch_bytes.json")

SPLIT_K = (0, 1, 2, 4)
K_GROUP = (0, 1, -1, -4)
DTYPE = (0, 1)

# shapes: (batch, hs, c0, c1, cout, stride, upsample)
GEMM = [(1, 64, 64, 0, 64, 1, 0), (2, 16, 128, 128, 128, 1, 2), (1, 32, 128, 0, 256, 2, 0)]
TINY = [(1, 4, 512, 0, 512, 1, 0), (1, 2, 512, 0, 512, 1, 1), (1, 8, 512, 0, 512, 2, 0)]
FULLK = [(2, 8, 512, 0, 512, 1, 0), (2, 8, 256, 256, 512, 1, 0), (2, 4, 512, 0, 512, 1, 1)]
ROW64 = [(1, 64, 64, 0, 64, 1, 0), (2, 128, 64, 0, 64, 1, 0), (1, 256, 64, 0, 64, 1, 0)]
ROW128 = [(1, 32, 128, 0, 128, 1, 0), (2, 64, 128, 0, 128, 1, 0), (1, 128, 128, 0, 128, 1, 0)]
BAND = [(8, 16, 512, 0, 512, 1, 0), (8, 8, 512, 0, 256, 1, 0), (16, 16, 512, 0, 64, 1, 0)]
ROWUP = [(4, 64, 128, 128, 64, 1, 2), (8, 128, 128, 128, 64, 1, 2), (2, 256, 128, 128, 64, 1, 2)]
WINO = [(1, 64, 256, 0, 256, 1, 0), (2, 32, 512, 0, 512, 1, 0), (1, 128, 128, 0, 128, 1, 0)]
WINOUP = [(1, 32, 256, 256, 256, 1, 2), (1, 64, 128, 128, 128, 1, 2), (2, 8, 512, 512, 512, 1, 1)]
PATCH = [(1, 64, 128, 0, 128, 1, 0), (2, 32, 256, 0, 256, 1, 0), (4, 64, 256, 0, 128, 1, 0)]
PATCHUP = [(1, 64, 64, 64, 128, 1, 2), (2, 32, 128, 128, 128, 1, 2), (4, 16, 256, 256, 256, 1, 2)]

CODES = [
    ((0, 0), GEMM), ((64, 64), GEMM), ((1, 1), TINY), ((16, 16), FULLK), ((32, 16), FULLK),
    ((1008, 64), ROW64), ((1008, 128), ROW128), ((2000, 32), BAND), ((3008, 64), ROWUP),
    ((4001, 0), WINO), ((4002, 0), WINO), ((4003, 0), WINO), ((5001, 0), WINOUP), ((5002, 0), WINOUP), ((6001, 0), WINO),
    ((7064, 128), PATCH), ((7064, 65), PATCH), ((7032, 128), PATCH), ((7164, 128), PATCHUP), ((7132, 128), PATCHUP), ((7116, 128), PATCHUP),
    ((7064, 64), PATCH), ((7032, 64), PATCH), ((7116, 64), PATCHUP),
]


def keys(tile):
    """(split_k, k_group, dtype) of a case's results, in order"""
    k_group = [k for k in K_GROUP if not (k == -1 and tile[0] > 7000 and tile[1] == 64)]
    return list(itertools.product(SPLIT_K, k_group, DTYPE))


def grid():
    """[(tile, shape)] in the order of the golden file's cases; each case holds one result per keys(tile), split_k slowest."""
    return [(tile, shape) for tile, shapes in CODES for shape in shapes]


def sweep(lib, tile, shape):
    b, hs, c0, c1, cout, stride, up = shape
    return [int(lib.lspf2f_conv3x3_scratch_bytes(b, hs, hs, c0, c1, cout, stride, up, tile[0], tile[1], sp, kg, dt))
            for sp, kg, dt in keys(tuple(tile))]


def test_scratch_bytes_equal_the_recorded_values():
    from livespeechportraits_amd import _native as N
    lib = N.load()
    gold = json.load(open(GOLDEN))
    assert (tuple(gold["split_k"]), tuple(gold["k_group"]), tuple(gold["dtype"])) == (SPLIT_K, K_GROUP, DTYPE)
    assert [(tuple(c["tile"]), tuple(c["shape"])) for c in gold["cases"]] == grid()          # the file covers the whole grid, in order
    assert len({tuple(c["bytes"]) for c in gold["cases"]}) > len(CODES)                     # ... and is no table of zeros
    for c in gold["cases"]:
        got = sweep(lib, c["tile"], c["shape"])
        assert len(c["bytes"]) == len(got)
        diff = [(k, g, w) for k, g, w in zip(keys(tuple(c["tile"])), got, c["bytes"]) if g != w]
        assert not diff, "tile %s shape %s: (split_k, k_group, dtype), got, recorded = %s" % (c["tile"], c["shape"], diff[:4])
