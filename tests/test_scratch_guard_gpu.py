"""GPU test of the stream-ordered scratch guard (csrc/common.h, RkScratch) on its success path: each of the seven entry points
that take their temporaries from it is called 20 times in a row on one stream, at the smallest shape of its own kernel test,
and must give the first call's outputs every time -- a buffer handed back too early, or handed out twice, would show as a
changed output.  Every comparison is exact: the outputs are integers, or floats whose value does not depend on the order of
addition (rk_heur_item_stats sums integer ratings, exact in float64 in any order; rk_build_norm_adj's values are per-entry).
The error paths are not provoked here; they are the destructor, read in common.h."""
import ctypes as C

import numpy as np
import pytest
import torch

from recad_amd import _lib
from recad_amd.graph import CsrGraph

from .test_attacker_kernels_gpu import _addr, _csr, _eligible_case
from .test_defender_kernels_gpu import Out, _call, _dev, _transpose_case
from .test_defender_kernels_gpu import _csr as _pca_csr
from .test_heuristic_kernels_gpu import dev_popular, dev_stats

pytestmark = pytest.mark.gpu
REPEATS = 20


def _eligible(dev):
    I, F, rows, excl = _eligible_case("n3")
    ptr, col, val = _csr(rows)
    U = len(rows)
    d = [_dev(ptr, dev), _addr(col, dev, np.int32), _addr(val, dev, np.float32), _dev(excl, dev)]
    L, P, S = _call()

    def call():
        pool_ptr, pool_col, el = Out(U + 1, torch.int32, dev), Out(len(col), torch.int32, dev), Out(U, torch.int32, dev)
        n_el = C.c_int32(-5)
        _lib.check(L.rk_aush_eligible(U, P(d[0]), P(d[1]), P(d[2]), P(d[3]), len(excl), F, P(pool_ptr.full), P(pool_col.full),
                                      P(el.full), C.byref(n_el), S(dev)), "rk_aush_eligible")
        return pool_ptr.host(), pool_col.host(), el.host(), np.int32(n_el.value)
    return call


def _permute(dev):
    n = 7
    src = _dev((np.random.default_rng(n).permutation(3 * n)[:n] + 7).astype(np.int32), dev)
    L, P, S = _call()

    def call():
        out = Out(n, torch.int32, dev)
        _lib.check(L.rk_aush_permute(n, P(src), 0x1234ABCD5678, 3, P(out.full), S(dev)), "rk_aush_permute")
        return (out.host(),)
    return call


def _item_stats(dev):
    rng = np.random.default_rng(9)
    col, val = rng.integers(0, 9, size=40), rng.integers(1, 6, size=40).astype(np.float32)      # integer ratings: exact sums
    return lambda: tuple(np.asarray(a) for a in dev_stats(dev, 9, col, val))


def _popular(dev):
    counts = np.array([3, 0, 5, 5, 1, 0, 2, 5, 4])                                                # 9 items, ties, unrated items

    def call():
        rc, ids, cs, n = dev_popular(dev, counts, 4)
        assert rc == 0 and n == 4
        return ids, cs
    return call


def _transpose(dev):
    n_rows, n_cols, rows = _transpose_case("ncols2")
    ptr, col, _ = _pca_csr(rows, n_rows)
    nnz = len(col)
    assert nnz > 0
    d = [_dev(ptr, dev), _dev(col, dev), _dev((np.random.default_rng(5).permutation(nnz) + 1).astype(np.float32), dev)]
    L, P, S = _call()

    def call():
        t_ptr, t_col, t_val = Out(n_cols + 1, torch.int32, dev), Out(nnz, torch.int32, dev), Out(nnz, torch.float32, dev)
        _lib.check(L.rk_pca_transpose(n_rows, n_cols, P(d[0]), P(d[1]), P(d[2]), P(t_ptr.full), P(t_col.full), P(t_val.full), S(dev)),
                   "rk_pca_transpose")
        return t_ptr.host(), t_col.host(), t_val.host()
    return call


def _select(dev):
    n = 12
    dist = _dev(np.random.default_rng(12).choice(np.array([-3.0, -0.0, 0.0, 2.0, 7.0], dtype=np.float32), n), dev)
    L, P, S = _call()

    def call():
        order = Out(n, torch.int32, dev)
        _lib.check(L.rk_pca_select(n, P(dist), n, P(order.full), S(dev)), "rk_pca_select")
        return (order.host(),)
    return call


def _norm_adj(dev):
    rows = [[0, 2, 6], [1], [], [0, 1, 2, 3, 4, 5, 6], [6]]                                        # 5 users, 7 items, 13 edges
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    idx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows])

    def call():
        g = CsrGraph.from_user_item_csr(5, 7, ptr, idx, dev)
        return g.rowptr.cpu().numpy(), g.col.cpu().numpy(), g.val.cpu().numpy()
    return call


@pytest.mark.parametrize("entry", [_eligible, _permute, _item_stats, _popular, _transpose, _select, _norm_adj],
                         ids=lambda f: f.__name__.lstrip("_"))
def test_repeated_calls_give_the_first_call_s_outputs(gpu_device, entry):
    call = entry(gpu_device)
    first = call()
    assert any(a.size for a in first)
    for rep in range(1, REPEATS):
        again = call()
        assert len(again) == len(first)
        for k, (a, b) in enumerate(zip(first, again)):
            assert a.dtype == b.dtype and np.array_equal(a, b), (rep, k)
