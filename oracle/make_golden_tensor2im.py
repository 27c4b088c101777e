#!/usr/bin/env python3
"""tensor2im fixture from the REFERENCE's own util.tensor2im (util/util.py), executed unmodified on a seeded [3, 17, 19]
input that covers the clipping range on both sides; asserts oracle/tensor2im_oracle.py bit-identical to it and freezes
input and output into tests/golden/tensor2im_u3_17x19.npz.  Usage: make_golden_tensor2im.py REFERENCE_TREE [--out DIR]"""
import argparse
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle.tensor2im_oracle import tensor2im      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ref", help="root of the reference source tree")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, a.ref)
    from util import util as ref_util              # the reference module
    x = np.random.default_rng(3).uniform(-1.2, 1.2, (3, 17, 19)).astype(np.float32)
    out = ref_util.tensor2im(torch.from_numpy(x))
    assert out.dtype == np.uint8 and np.array_equal(out, tensor2im(x)), "oracle/tensor2im_oracle.py deviates from the reference"
    np.savez(os.path.join(a.out, "tensor2im_u3_17x19.npz"), x=x, out=out)
    print("tensor2im_u3_17x19 ok: %d of %d values clipped" % (int(((out == 0) | (out == 255)).sum()), out.size))


if __name__ == "__main__":
    main()
