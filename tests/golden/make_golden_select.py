"""Generate tests/golden/select.npz FROM THE REFERENCE ITSELF.

Run in the authoring container only (needs /root/reference, which does not exist on the GPU box):

    python tests/golden/make_golden_select.py

It imports /root/reference/blocksparse/transformer.py behind the fake ``tensorflow`` of make_golden_bst.py (only the NumPy functions
``rectified_top_k_test``, ``masked_top_k_softmax_test``, ``masked_softmax_test`` and ``masked_softmax_grad_test`` are executed) and stores
their inputs and outputs for a dozen small seeded cases.  The reference orders by ``np.argsort``, which leaves ties open, so the softmax
cases hold distinct values; the ``rectified_top_k`` cases with ``rebase=True`` also hold tied ones, where a tie cannot change the result
(equal values above the k-th are all kept, equal values at the k-th all give 0).  No case has a row without an unmasked element: there the
reference stores 1 / k and this library zeros (include/bsmm_select.h).  ``sparse_relu`` is not in the fixture: blocksparse/lstm.py needs
more of tensorflow than the fake provides; tests/_select_ref.py pins it in float64.  Nothing at test time reads /root/reference.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_bst  # noqa: E402

# op, x shape, k, mask pattern (None, "row", "time", "head"), scale, rebase, tied
CASES = [
    ("rect", (6, 10), 3, None, 1.0, 1, 0),
    ("rect", (5, 33), 7, None, 1.0, 0, 0),
    ("rect", (4, 64), 17, None, 1.0, 1, 1),
    ("rect", (3, 100), 1, None, 1.0, 1, 1),
    ("topk", (2, 3, 5, 10), 4, None, 1.0, 0, 0),
    ("topk", (2, 3, 5, 24), 5, "row", 0.5, 0, 0),
    ("topk", (2, 3, 5, 40), 17, "time", 0.25, 0, 0),
    ("topk", (2, 3, 5, 65), 2, "head", 2.0, 0, 0),
    ("softmax", (7, 31), 31, None, 0.125, 0, 0),
    ("softmax", (2, 3, 5, 12), 12, "row", 1.0, 0, 0),
    ("softmax", (2, 3, 5, 20), 20, "time", 0.5, 0, 0),
    ("softmax", (2, 3, 5, 9), 9, "head", 1.0, 0, 0),
]


def make_mask(shape, pattern, rng):
    """A float mask of zeros and non-zero factors with at least one unmasked element in every row."""
    B, H, T, K = shape
    mshape = {"row": (1, 1, 1, K), "time": (1, 1, T, K), "head": (1, H, T, K)}[pattern]
    m = np.where(rng.random(mshape) < 0.4, 0.0, rng.choice([1.0, 0.5, 2.0], mshape)).astype(np.float32)
    m[..., rng.randint(0, K)] = 1.0
    return m


def main():
    tr = make_golden_bst.import_reference_transformer()
    out = {"ops": np.array([c[0] for c in CASES]), "ks": np.array([c[2] for c in CASES], dtype=np.int64),
           "scales": np.array([c[4] for c in CASES], dtype=np.float32), "rebase": np.array([c[5] for c in CASES], dtype=np.int64)}
    for i, (op, shape, k, pattern, scale, rebase, tied) in enumerate(CASES):
        rng = np.random.RandomState(700 + i)
        K = shape[-1]
        rows = int(np.prod(shape[:-1]))
        if tied:
            X = rng.choice(np.array([2.0, 1.0, 0.5, -0.5, -1.0], dtype=np.float32), (rows, K))
        else:                                            # distinct fp16 values: a shuffled ramp
            ramp = ((np.arange(K) - K / 3.0) / 8.0).astype(np.float16).astype(np.float32)
            X = np.stack([rng.permutation(ramp) for _ in range(rows)])
        X = X.reshape(shape).astype(np.float32)
        key = "c%d/" % i
        out[key + "X"] = X.astype(np.float16)
        M = None
        if pattern is not None:
            M = make_mask(shape, pattern, rng)
            out[key + "M"] = M
        if op == "rect":
            Y = tr.rectified_top_k_test(X, k, rebase=bool(rebase))
        elif op == "topk":
            Y = tr.masked_top_k_softmax_test(X, k, mask=M, scale=scale)
        else:
            Y = tr.masked_softmax_test(X, mask=M, scale=scale)
        out[key + "Y"] = np.asarray(Y, dtype=np.float32)
        if op != "rect":
            DY = rng.normal(0.0, 1.0, shape).astype(np.float16).astype(np.float32)
            out[key + "DY"] = DY.astype(np.float16)
            out[key + "DX"] = np.asarray(tr.masked_softmax_grad_test(DY, out[key + "Y"], mask=M, scale=scale), dtype=np.float32)
    path = os.path.join(HERE, "select.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
