"""Random CSR slabs shared by the SpMM tests (test_gpu_parity.py, test_sharded_ops_*.py).  Test infrastructure only."""
import numpy as np


def _rand_csr(rng, n, avg, long_rows=(), n_cols=None):
    """n rows of Poisson(avg) nonzeros (long_rows: (row, count) overrides, 0 = an empty row), sorted distinct columns below
    n_cols (default n: a square slab), values uniform in [0, 1)."""
    n_cols = n if n_cols is None else n_cols
    deg = rng.poisson(avg, n).astype(np.int64)
    for r, k in long_rows:
        deg[r] = k
    deg = np.minimum(deg, n_cols)
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(deg)
    col = np.concatenate([np.sort(rng.choice(n_cols, size=k, replace=False)) for k in deg]).astype(np.int32)
    val = rng.random(len(col), dtype=np.float32)
    return rowptr, col, val
