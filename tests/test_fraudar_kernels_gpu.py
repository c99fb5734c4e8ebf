"""GPU tests of the FraudarSelectUsers kernels one entry point at a time (csrc/fraudar.hip) against the restatement of the
definition on Python integers (tests/_fraudar_restate.py).  Every entry runs from inputs the test owns; everything is compared
word for word: no tolerance, no excluded case.  Every output buffer is pre-filled with a sentinel and carries a 64-element
margin that must stay as it was.  uint32 / uint64 words travel in int32 / int64 tensors."""
import functools

import numpy as np
import pytest
import torch

from recad_amd import _lib, synth
from tests import _fraudar_restate as R

pytestmark = pytest.mark.gpu
MARGIN, SENTINEL = 64, -777
EINVAL = -22


class Out:
    """A device buffer of n elements followed by MARGIN more, all SENTINEL."""

    def __init__(self, n, dtype, dev):
        self.n = int(n)
        self.full = torch.full((self.n + MARGIN,), SENTINEL, dtype=dtype, device=dev)

    def host(self):
        assert (self.full[self.n:].cpu().numpy() == SENTINEL).all(), "the kernel wrote past the end of its output"
        return self.full[: self.n].cpu().numpy()

    def untouched(self):
        return bool((self.full.cpu().numpy() == SENTINEL).all())


def _dev(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(dev)     # an empty array still needs an address


def _csr_of(A):
    ptr = np.concatenate([[0], np.cumsum(A.sum(axis=1))]).astype(np.int32)
    return ptr, np.nonzero(A)[1].astype(np.int32)


def _transpose(ptr, idx, n_items):
    """colptr / crow as rk_pca_transpose writes them: users ascending inside a column."""
    row = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    o = np.lexsort((row, idx))
    colptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n_items))]).astype(np.int32)
    return colptr, row[o].astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- rk_fd_init
def _init(dev, U, I, ptr, idx, wtab):
    o = {"w_item": Out(I, torch.int32, dev), "pri": Out(U + I, torch.int64, dev), "info": Out(4, torch.int64, dev),
         "status": Out(2, torch.int32, dev)}
    colptr, _ = _transpose(ptr, idx, I)
    d = [_dev(a, dev) for a in (ptr, idx, colptr, np.asarray(wtab, dtype=np.uint32).view(np.int32))]
    L, P = _lib.lib(), _lib.ptr
    rc = L.rk_fd_init(U, I, len(idx), P(d[0]), P(d[1]), P(d[2]), P(d[3]), P(o["w_item"].full), P(o["pri"].full), P(o["info"].full),
                      P(o["status"].full), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, o


def _init_graph(U, I, rng, empty_rows):
    """Random columns, column 0 rated by every user, a few empty columns; then the first, middle and last row emptied."""
    A = rng.random((U, I)) < rng.random(I)[None, :]
    A[:, rng.permutation(I)[: I // 5]] = False
    A[:, 0] = True
    if empty_rows:
        A[[0, U // 2, U - 1]] = False
    return _csr_of(A)


@pytest.mark.parametrize("U", [1, 5, 70, 300])
def test_init(gpu_device, U):
    rng = np.random.default_rng(U)
    for I in (1, 63, 64, 65, 200):
        for empty_rows in (False, True):
            ptr, idx = _init_graph(U, I, rng, empty_rows)
            for kind in ("log", "degree"):
                wtab = R.weight_table(U, kind)
                want_w, want_pri, want_f0 = R.init(U, I, ptr, idx, wtab)
                rc, o = _init(gpu_device, U, I, ptr, idx, wtab)
                assert rc == 0 and o["status"].host().tolist() == [0, -1], (U, I, kind)
                assert np.array_equal(o["w_item"].host().view(np.uint32), want_w), (U, I, kind)
                assert np.array_equal(o["pri"].host().view(np.uint64), want_pri), (U, I, kind)
                assert o["info"].host().tolist() == [SENTINEL] * 3 + [want_f0], (U, I, kind)
                assert want_f0 == int(want_pri[:U].sum()) and (empty_rows or int(want_pri[U]) == U * int(want_w[0]))


def test_init_refusals(gpu_device):
    """A table entry of 0 and one of 2^24 + 1, each at two degrees some item has: refused at the lower one, nothing written;
    the same entries at degrees no item has are not met."""
    U, I = 70, 65
    ptr, idx = _init_graph(U, I, np.random.default_rng(5), False)
    met = sorted(set(R.degrees(idx, I).tolist()))
    unmet = [d for d in range(U + 1) if d not in met]
    assert len(met) > 6 and 0 in met and len(unmet) > 3
    for bad in (0, R.ONE + 1, 2 ** 32 - 1):
        wtab = R.weight_table(U, "log")
        wtab[[met[3], met[5]]] = bad
        assert R.init(U, I, ptr, idx, wtab) == ("refused", R.BAD_WEIGHT, met[3])
        rc, o = _init(gpu_device, U, I, ptr, idx, wtab)
        assert rc == EINVAL and o["status"].host().tolist() == [R.BAD_WEIGHT, met[3]]
        assert o["w_item"].untouched() and o["pri"].untouched() and o["info"].untouched(), "outputs must be untouched after a refusal"
        msg = _lib.lib().rk_last_error().decode()
        assert f"rule {R.BAD_WEIGHT}" in msg and f"wtab[{met[3]}]" in msg
        wtab = R.weight_table(U, "log")
        wtab[unmet] = bad
        rc, o = _init(gpu_device, U, I, ptr, idx, wtab)
        assert rc == 0 and np.array_equal(o["w_item"].host().view(np.uint32), R.init(U, I, ptr, idx, wtab)[0])
    wtab = R.weight_table(U, "log")
    wtab[0] = 0                                                        # an unrated item meets wtab[0]
    assert _init(gpu_device, U, I, ptr, idx, wtab)[1]["status"].host().tolist() == [R.BAD_WEIGHT, 0]
    # argument refusals: nothing launched, nothing written
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(gpu_device)
    z = torch.zeros(600, dtype=torch.int32, device=gpu_device)
    o = [Out(8, torch.int32, gpu_device), Out(16, torch.int64, gpu_device), Out(4, torch.int64, gpu_device), Out(2, torch.int32, gpu_device)]
    for u, i, nnz in ((-1, 8, 0), (8, -1, 0), (0, 0, 0), (_lib.RK_FD_MAX_NODES, 1, 0), (8, 8, -1), (8, 8, _lib.RK_FD_MAX_NNZ)):
        assert L.rk_fd_init(u, i, nnz, P(z), P(z), P(z), P(z), P(o[0].full), P(o[1].full), P(o[2].full), P(o[3].full), s) == EINVAL
    assert L.rk_fd_init(8, 8, 0, P(z), P(z), None, P(z), P(o[0].full), P(o[1].full), P(o[2].full), P(o[3].full), s) == EINVAL
    assert L.rk_fd_init(8, 8, 0, P(z), P(z), P(z), P(z), P(o[0].full), None, P(o[2].full), P(o[3].full), s) == EINVAL
    torch.cuda.synchronize()
    assert all(x.untouched() for x in o)


# ---------------------------------------------------------------------------------------------------------------- rk_fd_peel
def _priorities(U, I, ptr, idx, w):
    """The definition's initial priorities for any weights, as uint64 [U + I]."""
    w = np.asarray(w, dtype=np.uint64)
    pri = np.zeros(U + I, dtype=np.uint64)
    if len(idx):
        np.add.at(pri, np.repeat(np.arange(U), np.diff(ptr)), w[idx])
    pri[U:] = w * np.bincount(idx, minlength=I).astype(np.uint64)
    return pri


def _peel(dev, U, I, ptr, idx, w, steps_per_launch=None, trace=True):
    N = U + I
    o = {"order": Out(N, torch.int32, dev), "step_of": Out(N, torch.int32, dev), "f_trace": Out(N, torch.int64, dev),
         "info": Out(4, torch.int64, dev)}
    colptr, crow = _transpose(ptr, idx, I)
    pri = Out(N, torch.int64, dev)
    pri.full[:N] = _dev(_priorities(U, I, ptr, idx, w).view(np.int64), dev)[:N]
    d = [_dev(a, dev) for a in (ptr.astype(np.int32), idx.astype(np.int32), colptr, crow, np.asarray(w, dtype=np.uint32).view(np.int32))]
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(dev)
    args = (U, I, len(idx), P(d[0]), P(d[1]), P(d[2]), P(d[3]), P(d[4]), P(pri.full), P(o["order"].full), P(o["step_of"].full),
            P(o["f_trace"].full) if trace else None, P(o["info"].full))
    rc = L.rk_fd_peel(*args, s) if steps_per_launch is None else L.rk_fd_peel_ex(*args, steps_per_launch, s)
    torch.cuda.synchronize()
    o["pri"] = pri
    return rc, o


def _check_peel(dev, U, I, ptr, idx, w, want=None, **kw):
    want = want or R.peel(U, I, ptr, idx, w)
    rc, o = _peel(dev, U, I, ptr, idx, w, **kw)
    assert rc == 0
    assert np.array_equal(o["order"].host(), want[0]), "order"
    assert np.array_equal(o["step_of"].host(), want[1]), "step_of"
    if kw.get("trace", True):
        assert np.array_equal(o["f_trace"].host().view(np.uint64), want[2]), "f_trace"
    else:
        assert o["f_trace"].untouched()
    assert o["info"].host().tolist() == list(want[3]) + [int(want[2][0])], "info"
    assert (o["pri"].host() == -1).all(), "every node ends removed: 2^64 - 1"
    return want, o


def _sparse(U, I, n_edges, seed):
    rng = np.random.default_rng(seed)
    A = np.zeros((U, I), dtype=bool)
    if U and I:
        A[rng.integers(0, U, size=n_edges), rng.integers(0, I, size=n_edges)] = True
    return _csr_of(A)


@pytest.mark.parametrize("U,I,n_edges", [(1, 0, 0), (0, 1, 0), (1, 1, 1), (40, 23, 300), (40, 24, 300), (40, 25, 300), (4000, 95, 3000),
                                         (4000, 96, 3000), (4000, 97, 3000), (4000, 200, 5000)])
def test_peel_around_the_level_edges(gpu_device, U, I, n_edges):
    """N = 1, 2, 63..65 (one leaf block / two), 4095..4097 (two levels / three), 4200."""
    ptr, idx = _sparse(U, I, n_edges, U + I)
    for kind in ("log", "degree"):
        w = R.weight_table(U, kind)[R.degrees(idx, I)]
        _check_peel(gpu_device, U, I, ptr, idx, w)


ROW_LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025)


def test_peel_row_and_column_lengths(gpu_device):
    """Rows and columns of 0, 1, 63..65 and 1023..1025 entries (the workgroup strides 256 at a time) in a 1 100 x 1 100 graph."""
    rng = np.random.default_rng(11)
    n = 1100
    A = rng.random((n, n)) < 0.002
    for k, length in enumerate(ROW_LENGTHS):
        A[k] = False
        A[:, k] = False
    for k, length in enumerate(ROW_LENGTHS):
        A[k, 8 + rng.permutation(n - 8)[:length]] = True
        A[8 + rng.permutation(n - 8)[:length], k] = True
    ptr, idx = _csr_of(A)
    assert np.diff(ptr)[:8].tolist() == list(ROW_LENGTHS) and R.degrees(idx, n)[:8].tolist() == list(ROW_LENGTHS)
    w = R.weight_table(n, "log")[R.degrees(idx, n)]
    _check_peel(gpu_device, n, n, ptr, idx, w)


def test_peel_ties_inside_and_across_leaf_blocks(gpu_device):
    """200 identical users on the same 100 items beside 150 identical users on 70 others, unit weights: whole runs of equal
    priorities that span leaf blocks; then K_70,70, where every priority is equal from the start."""
    A = np.zeros((350, 170), dtype=bool)
    A[:200, :100] = True
    A[200:, 100:] = True
    ptr, idx = _csr_of(A)
    want, _ = _check_peel(gpu_device, 350, 170, ptr, idx, np.full(170, R.ONE, dtype=np.uint32))
    assert want[3][0] > 0
    ptr, idx = _csr_of(np.ones((70, 70), dtype=bool))
    want, _ = _check_peel(gpu_device, 70, 70, ptr, idx, np.full(70, R.ONE, dtype=np.uint32))
    assert want[3] == (0, 4900 * R.ONE, 140) and want[0][0] == 0


@functools.lru_cache(maxsize=None)
def _planted():
    """synth `tiny` plus 40 users (ids 300...) who all rate the 40 least-rated items."""
    d = synth.make("tiny")
    ptr, idx = (np.asarray(a) for a in d["train"])
    ptr, idx = ptr[:301].astype(np.int64), idx[: ptr[300]].astype(np.int64)
    items = np.sort(np.argsort(R.degrees(idx, 200), kind="stable")[:40])
    ptr, idx = np.concatenate([ptr, ptr[-1] + 40 * np.arange(1, 41)]), np.concatenate([idx] + [items] * 40)
    w = R.weight_table(340, "log")[R.degrees(idx, 200)]
    return ptr, idx, w, R.peel(340, 200, ptr, idx, w)


def test_peel_planted_block_and_launch_edges(gpu_device):
    ptr, idx, w, want = _planted()
    N = 540
    assert want[3][0] == 460 and want[3][2] == 80
    _, first = _check_peel(gpu_device, 340, 200, ptr, idx, w, want=want)
    for spl in (1, 7, 64, N, N + 5):
        _check_peel(gpu_device, 340, 200, ptr, idx, w, want=want, steps_per_launch=spl)
    _, again = _check_peel(gpu_device, 340, 200, ptr, idx, w, want=want)
    assert all(torch.equal(first[k].full, again[k].full) for k in first), "the same call twice gives the same bits"
    _check_peel(gpu_device, 340, 200, ptr, idx, w, want=want, trace=False)
    _check_peel(gpu_device, 340, 200, ptr, idx, w, want=want, trace=False, steps_per_launch=7)


def test_peel_launch_edges_on_three_levels(gpu_device):
    ptr, idx = _sparse(4000, 200, 5000, 3)
    w = R.weight_table(4000, "log")[R.degrees(idx, 200)]
    want = R.peel(4000, 200, ptr, idx, w)
    for spl in (7, 64, 4095, 4205):
        _check_peel(gpu_device, 4000, 200, ptr, idx, w, want=want, steps_per_launch=spl)


def test_peel_carries(gpu_device):
    """A dense 300 x 200 block at hand-made weights of 2^24 plus a tail of isolated nodes: the items' priorities pass 2^32 (the
    borrow of the 64-bit subtraction).  f * n stays below 2^64 there (60 000 * 2^24 * N with N <= 2^19), so the same block at
    hand-made weights of 2^32 - 1 with 100 000 nodes follows: f_0 * N is about 2^64.5 and the comparison needs its high word."""
    A = np.zeros((2300, 1200), dtype=bool)
    A[:300, :200] = True
    ptr, idx = _csr_of(A)
    want, _ = _check_peel(gpu_device, 2300, 1200, ptr, idx, np.full(1200, R.ONE, dtype=np.uint32))
    assert want[3] == (3000, 60000 * R.ONE, 500) and 300 * R.ONE > 2 ** 32
    U, I = 60000, 40000
    ptr = np.concatenate([200 * np.arange(301), np.full(U - 300, 60000)]).astype(np.int64)
    idx = np.tile(np.arange(200), 300).astype(np.int64)
    w = np.full(I, 2 ** 32 - 1, dtype=np.uint32)
    want, _ = _check_peel(gpu_device, U, I, ptr, idx, w)
    assert int(want[2][0]) * (U + I) > 2 ** 64 and want[3] == (U + I - 500, 60000 * (2 ** 32 - 1), 500)


def test_peel_refusals(gpu_device):
    ptr, idx, w, _ = _planted()
    rc, o = _peel(gpu_device, 340, 200, ptr, idx, w, steps_per_launch=0)
    assert rc == EINVAL and all(o[k].untouched() for k in ("order", "step_of", "f_trace", "info"))
    assert _peel(gpu_device, 340, 200, ptr, idx, w, steps_per_launch=-3)[0] == EINVAL
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(gpu_device)
    z = torch.zeros(600, dtype=torch.int32, device=gpu_device)
    z64 = torch.zeros(16, dtype=torch.int64, device=gpu_device)
    o = [Out(16, torch.int32, gpu_device), Out(16, torch.int32, gpu_device), Out(16, torch.int64, gpu_device), Out(4, torch.int64, gpu_device)]
    out = (P(o[0].full), P(o[1].full), P(o[2].full), P(o[3].full))
    for u, i, nnz in ((-1, 8, 0), (8, -1, 0), (0, 0, 0), (_lib.RK_FD_MAX_NODES, 1, 0), (1, _lib.RK_FD_MAX_NODES, 0), (8, 8, -1),
                      (8, 8, _lib.RK_FD_MAX_NNZ)):
        assert L.rk_fd_peel(u, i, nnz, P(z), P(z), P(z), P(z), P(z), P(z64), *out, s) == EINVAL, (u, i, nnz)
        assert L.rk_fd_peel_ex(u, i, nnz, P(z), P(z), P(z), P(z), P(z), P(z64), *out, 64, s) == EINVAL, (u, i, nnz)
    for missing in range(6):
        a = [P(z), P(z), P(z), P(z), P(z), P(z64)]
        a[missing] = None
        assert L.rk_fd_peel(8, 8, 0, *a, *out, s) == EINVAL, missing
    for missing in (0, 1, 3):
        b = list(out)
        b[missing] = None
        assert L.rk_fd_peel(8, 8, 0, P(z), P(z), P(z), P(z), P(z), P(z64), *b, s) == EINVAL, missing
    torch.cuda.synchronize()
    assert all(x.untouched() for x in o) and bool((z64 == 0).all())
