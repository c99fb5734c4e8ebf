"""Randomised sweep of the fp32 MFMA GEMM through rk_gemm_f32: M, N in [1, 400], K in [1, 300], one of the three operand
layouts (forward: A and B k-contiguous; dX: B row-contiguous; dW: both row-contiguous), an epilogue, an optional row gather
and an optional K-split (atomics or parked slices), compared by the rules of tests/_gemm_forms.py (bit-exact against the
oracle's k-ordered chain; the derived bound for the atomics; guards untouched).  Prints and returns the forms it reached."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import _gemm_forms as GF   # noqa: E402

LAYOUTS = (("k", "k"), ("k", "r"), ("r", "r"))
EPILOGUES = (dict(), dict(col_bias=True), dict(col_bias=True, relu=True), dict(row_bias=True, col_bias=True, const_add=0.5),
             dict(mask=True), dict(col_bias=True, relu=True, mask=True), dict(sigmoid=True), dict(keep_prob=0.75))


def run(seed=0, n_cases=100):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    forms = set()
    for case in range(n_cases):
        M, N, K = int(rng.integers(1, 401)), int(rng.integers(1, 401)), int(rng.integers(1, 301))
        if rng.random() < 0.3:   # whole tiles and chunks now and then: the vector-load paths and the deep form
            M, N, K = (M + 63) // 64 * 64, (N + 63) // 64 * 64, (K + 127) // 128 * 128
        la, lb = LAYOUTS[int(rng.integers(0, 3))]
        kw = dict(la=la, lb=lb, seed=seed * 1000 + case, gates=False)
        kw["ldc"] = N + int(rng.integers(0, 2)) * int(rng.integers(1, 9))
        mode = int(rng.integers(0, 4))   # 0, 1: epilogue; 2: epilogue behind a row gather; 3: K-split
        if mode == 3:
            kw.update(split_k=int(rng.integers(2, 9)), parked=bool(rng.integers(0, 2)))
        else:
            kw.update(EPILOGUES[int(rng.integers(0, len(EPILOGUES)))])
            if mode == 2:
                kw["ridx"] = ("identity", "perm")[int(rng.integers(0, 2))]
        try:
            form, strip, _ = GF.run_case(dev, M, N, K, **kw)
        except AssertionError:
            print("MISMATCH case", case, dict(M=M, N=N, K=K, **kw))
            raise
        forms.update((form, strip))
    forms.discard(GF.NONE)
    print(f"{n_cases} cases ok; forms: {sorted(GF.name_of(f) for f in forms)}")
    return forms


if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 0, int(sys.argv[2]) if len(sys.argv) > 2 else 100)
