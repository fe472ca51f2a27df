"""Generate tests/golden/layer_norm.npz FROM THE REFERENCE ITSELF.

Run in the authoring container only (needs /root/reference, which does not exist on the GPU box):

    python tests/golden/make_golden_layer_norm.py

It imports /root/reference/blocksparse/norms.py behind the fake ``tensorflow`` of make_golden.py (only the NumPy functions
``layer_norm_test`` / ``layer_norm_grad_test`` are executed) and stores their inputs and outputs for a few small seeded cases: both axes,
one and several segments on both, ReLU on and off, and the (N, K) = (4, 31) / (4, 33) shapes of the reference's test/layer_norm_test.py.
Inputs are drawn as that test draws them -- N(0, 1) rounded through fp16, so they are stored as fp16 without loss -- and the reference
computes in fp32.  Nothing at test time reads /root/reference.
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

# K, N, axis, segments, relu
CASES = [
    (31, 4, 0, 1, 0),
    (33, 4, 1, 1, 0),
    (31, 4, 1, 1, 1),
    (33, 4, 0, 1, 1),
    (32, 4, 0, 1, 0),
    (40, 24, 0, 1, 0),
    (40, 21, 0, 2, 1),
    (64, 16, 0, 4, 0),
    (128, 5, 1, 4, 0),
    (36, 24, 1, 3, 1),
]


def main():
    make_golden.import_reference_matmul()             # installs the fake tensorflow and the `blocksparse` package path
    norms = importlib.import_module("blocksparse.norms")
    out = {"cases": np.array(CASES, dtype=np.int64)}
    for i, (K, N, axis, S, relu) in enumerate(CASES):
        rng = np.random.RandomState(500 + i)
        shape_x = (K, N) if axis == 0 else (N, K)
        shape_b = (K, 1) if axis == 0 else (1, K)       # test/layer_norm_test.py:60-65
        f16 = lambda a: a.astype(np.float16).astype(np.float32)
        X, E = f16(rng.normal(0.0, 1.0, shape_x)), f16(rng.normal(0.0, 1.0, shape_x))
        G, B = f16(rng.normal(0.0, 1.0, shape_b)), f16(rng.normal(0.0, 1.0, shape_b))
        Y = norms.layer_norm_test(X, G, B, axis=axis, segments=S, relu=bool(relu))
        DX, DG, DB = norms.layer_norm_grad_test(E, X, G, B, axis=axis, segments=S, relu=bool(relu))
        key = "c%d/" % i
        for name, a in (("X", X), ("E", E), ("G", G), ("B", B)):
            out[key + name] = a.astype(np.float16)
        for name, a in (("Y", Y), ("DX", DX), ("DG", DG), ("DB", DB)):
            out[key + name] = np.asarray(a, dtype=np.float32)
    path = os.path.join(HERE, "layer_norm.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
