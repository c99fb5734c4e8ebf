"""numpy restatement of the library's counter-based dropout (recad_amd/csrc/common.h: rk_mix64, rk_drop_step_seed,
rk_drop_keep), shared by the GPU test files that compare a kernel's dropout epilogue element by element."""
import numpy as np


def _mix64(z):
    """numpy mirror of rk_mix64 (recad_amd/csrc/common.h), uint64 wrap-around arithmetic"""
    with np.errstate(over="ignore"):
        z = (np.asarray(z, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _drop_keep(seed_step, n, keep_prob):
    """numpy mirror of rk_drop_keep (recad_amd/csrc/common.h) for element ids 0..n-1"""
    with np.errstate(over="ignore"):
        ids = np.arange(n, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95)
        u24 = _mix64(np.uint64(seed_step) ^ ids) >> np.uint64(40)
    return u24 < np.uint64(int((1.0 - (1.0 - float(keep_prob))) * 16777216.0))


def _step_seed(base, step):
    with np.errstate(over="ignore"):
        return int(_mix64(np.uint64(base) ^ _mix64(np.uint64(step))))
