"""GPU tests of what runs before and after the compute kernels, one entry point at a time through the C ABI: the samplers
(rk_bpr_sample, rk_pointwise_sample) against the numpy restatement of sampler.hip (tests/_sampler_restate.py), the graph
builders (rk_coo_to_csr, rk_build_norm_adj), the evaluation plumbing (rk_eligible_users, rk_pred_shift, rk_hit_counts) and
rk_pair_scores against restatements written here.  Every output is pre-filled with a sentinel (-7) and allocated a few elements
longer than the entry point may write, so an element left unwritten and a write past the end are both seen.

Shapes, and why each is there.
  rk_bpr_sample       sparse graph U = 300, I = 200, rows of 0..30 items, empty rows at both ends and in the middle, n_draws 1,
                      255, 256, 257 (around one 256-thread block) and 5000 (many blocks); the dense graph U = 8, I = 40 (rows of
                      39 items whose free item is the first, a middle and the last one, 38 items, the full row, an empty row, 1
                      and 20 items) at 4096 draws: the 64 rejections fail on a fifth of the 39-item draws, so rth_free_item
                      runs, and the full / empty rows take the valid = 0 exit; U = 1, I = 2, deg = 1 (the smallest graph with a
                      negative); 4096 * 256 + 777 draws (second turn of the grid-stride loop); n_draws = 0; null pointers.
  rk_pointwise_sample the sparse graph at ratio 0, 1, 4 (its empty users at the start, in the middle and at the end put equal
                      pointers under the edge-to-user search); the dense graph (one free item at the first, a middle and the
                      last position; the full user, whose negative rows are (u, 0, 0)); U = 600, I = 200, ratio 70 with
                      total > 8192 * 256 rows (stride loop).
  rk_coo_to_csr       n_rows 1, 255, 256, 257, 1000 (around one block of the row-pointer kernel) with empty rows at the start,
                      at the end and in runs; nnz = 0; nnz = 4096 * 256 + 3 (the copy kernel's stride loop); nnz < 0.
  rk_build_norm_adj   (U, I) = (1, 1), (5, 3), (301, 1023 / 1024 / 1025), (77, 2053): one, one full, two and three passes of the
                      1024-thread scan, U no multiple of the 4 waves of a block; users of more than 64 and more than 128 items
                      (second and third turn of a wave over its row); empty users; items nobody rated, the first and the last
                      included; E = 0; U = 3000, I = 1500 with E just above 8192 * 256 (stride loops of the count and the
                      item-row kernels).
  rk_eligible_users   n_users 1, 63, 64, 65 (one wave), 1023, 1024, 1025 (one pass of the compaction), 3000, and 2048 * 256 +
                      100 (second turn of the flag kernel's stride loop, 513 passes); 0, 1 and 4 targets, among them the first
                      and the last item of a row; nobody and everybody eligible.
  rk_pred_shift       n 0, 1, 1023, 1024, 1025 (around one element per thread), 100 003; +-1e6 values that cancel to 1e-3.
  rk_hit_counts       nk 1, 4, 5, 8 (one group of four thresholds, a padded second group, two groups), descending and repeated
                      cut-offs, T 1 and 3, n 1, 16 384, 16 385 (one block that stores / two that add atomically), 64 * 16 384 +
                      5 (the stride loop).
  rk_pair_scores      d 1, 63, 64, 65, 130, 256 (a wave's lanes partly used, once, twice, up to four times), n 1, 3, 4, 5
                      (around the four waves of a block) and 4096 * 4 + 9 (the wave-stride loop), repeated ids, with and
                      without biases, dropout 0, 0.25, 0.9.

Bounds.  None was measured for this file.  The samplers, rk_coo_to_csr, rk_eligible_users, rk_hit_counts, the index arrays of
rk_build_norm_adj, the symmetry of its values and the dropout mask are integers or bit patterns: equality.  rk_pred_shift adds
in double in a fixed order without a multiply, restated here in that order: equality.  The values of rk_build_norm_adj keep the
project's existing bound for this entry point, rtol 4e-7 per entry (device powf against the host's, test_norm_adj_on_device).
rk_pair_scores against float64 is derived: a term passes at most m = ceil(d / 64) + 6 + 3 + 2 fp32 roundings (the lane's chain,
six butterfly steps, three bias adds, the product and the dropout scale), each of relative size 2^-24, so the error is at most
m * 2^-24 * S with S = sum |u_k i_k| + |ub| + |ib| + |mean|; a kept output under dropout is S scaled by 1 / (1 - p) with it, and
is in addition bit-identical to the undropped device score times the fp32 scale, one more fp32 product."""
import math

import numpy as np
import pytest
import torch

from recad_amd import _lib
from recad_amd.evaluate import eligible_users

from . import _sampler_restate as S
from ._drop_restate import _drop_keep

pytestmark = pytest.mark.gpu
EINVAL = -22
SENT = -7
PAD = 5
BIG_SEED = 2 ** 61 + 12345


def _t(a, dtype, dev, pad=1):
    """device copy of a host array, `pad` zero elements longer (an empty array still has an address)"""
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    return torch.as_tensor(np.concatenate([a, np.zeros(pad, dtype=dtype)])).to(dev)


def _out(n, dtype, dev):
    return torch.full((n + PAD,), SENT, dtype=dtype, device=dev)


def _host(t, n):
    """(the first n elements, whether the PAD elements after them still hold the sentinel)"""
    a = t.cpu().numpy()
    return a[:n], bool((a[n:] == SENT).all())


# ---------------------------------------------------------------- rk_bpr_sample
def _bpr(dev, U, I, ptr, idx, n, seed, null=()):
    a = {"ptr": _t(ptr, np.int32, dev), "idx": _t(idx, np.int32, dev), "users": _out(n, torch.int64, dev),
         "pos": _out(n, torch.int64, dev), "neg": _out(n, torch.int64, dev), "valid": _out(n, torch.int32, dev)}
    p = {k: (None if k in null else _lib.ptr(v)) for k, v in a.items()}
    rc = _lib.lib().rk_bpr_sample(U, I, p["ptr"], p["idx"], n, seed, p["users"], p["pos"], p["neg"], p["valid"], _lib.stream_ptr())
    torch.cuda.synchronize()
    got = [_host(a[k], n) for k in ("users", "pos", "neg", "valid")]
    return rc, [g[0] for g in got], all(g[1] for g in got)


def _bpr_equals_restatement(dev, U, I, ptr, idx, n, seed):
    rc, got, tail = _bpr(dev, U, I, ptr, idx, n, seed)
    ref = S.bpr_sample(U, I, ptr, idx, n, seed)
    assert rc == 0 and tail, (n, seed)
    for name, g, r in zip(("users", "pos", "neg", "valid"), got, ref):
        assert np.array_equal(g, r), (name, n, seed, int(np.count_nonzero(g != r)))
    return ref


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_bpr_sample_sparse(gpu_device, n):
    ptr, idx = S.sparse_case()
    for seed in (12345, BIG_SEED):
        _bpr_equals_restatement(gpu_device, 300, 200, ptr, idx, n, seed)


def test_bpr_sample_dense_rows_take_the_fallback(gpu_device):
    ptr, idx = S.dense_case()
    for seed in (12345, BIG_SEED):
        users, pos, neg, valid, fb = _bpr_equals_restatement(gpu_device, 8, S.DENSE_I, ptr, idx, 4096, seed)
        assert fb.sum() > 0 and fb[users <= 2].sum() > 0
        assert np.array_equal(valid == 0, np.isin(users, [S.DENSE_ROWS["full"], S.DENSE_ROWS["empty"]])) and (valid == 0).any()


def test_bpr_sample_smallest_graph(gpu_device):
    for row, free in (([0], 1), ([1], 0)):
        ptr, idx = S.csr_of([row])
        for seed in (3, BIG_SEED):
            users, pos, neg, valid, _ = _bpr_equals_restatement(gpu_device, 1, 2, ptr, idx, 300, seed)
            assert (users == 0).all() and (pos == row[0]).all() and (neg == free).all() and valid.all()


def test_bpr_sample_grid_stride(gpu_device):
    ptr, idx = S.sparse_case()
    n = 4096 * 256 + 777
    for seed in (7, BIG_SEED):
        _bpr_equals_restatement(gpu_device, 300, 200, ptr, idx, n, seed)


def test_bpr_sample_empty_call_and_refusals(gpu_device):
    ptr, idx = S.sparse_case()
    dev = gpu_device
    # n_draws = 0 writes nothing at all: the outputs in front of the pad keep the sentinel too
    a = [_out(16, torch.int64, dev) for _ in range(3)] + [_out(16, torch.int32, dev)]
    ins = [_t(ptr, np.int32, dev), _t(idx, np.int32, dev)]
    rc = _lib.lib().rk_bpr_sample(300, 200, _lib.ptr(ins[0]), _lib.ptr(ins[1]), 0, 5, *(_lib.ptr(t) for t in a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and all(bool((t == SENT).all()) for t in a)
    for name in ("ptr", "idx", "users", "pos", "neg", "valid"):
        rc, got, tail = _bpr(gpu_device, 300, 200, ptr, idx, 64, 5, null=(name,))
        assert rc == EINVAL and tail and all((g == SENT).all() for g in got), name


# ---------------------------------------------------------------- rk_pointwise_sample
def _pointwise(dev, U, I, ptr, idx, ratio, seed):
    E = len(idx)
    n = E * (ratio + 1)
    outs = [_out(n, torch.int64, dev) for _ in range(3)]
    ins = [_t(ptr, np.int32, dev), _t(idx, np.int32, dev)]       # named, so that they outlive the call
    rc = _lib.lib().rk_pointwise_sample(U, I, _lib.ptr(ins[0]), _lib.ptr(ins[1]), E, ratio, seed, *(_lib.ptr(t) for t in outs),
                                        _lib.stream_ptr())
    torch.cuda.synchronize()
    got = [_host(t, n) for t in outs]
    ref = S.pointwise_sample(U, I, ptr, idx, ratio, seed)
    assert rc == 0 and all(g[1] for g in got), (ratio, seed)
    for name, g, r in zip(("users", "items", "labels"), got, ref):
        assert np.array_equal(g[0], r), (name, ratio, seed, int(np.count_nonzero(g[0] != r)))
    return ref


@pytest.mark.parametrize("ratio", [0, 1, 4])
def test_pointwise_sample_sparse_with_empty_users(gpu_device, ratio):
    ptr, idx = S.sparse_case()
    deg = np.diff(ptr)
    assert not deg[:3].any() and not deg[-2:].any() and deg[150] == 0 and deg[3] > 0
    for seed in (12345, BIG_SEED):
        users, items, labels = _pointwise(gpu_device, 300, 200, ptr, idx, ratio, seed)
        assert np.array_equal(users[:: ratio + 1], np.repeat(np.arange(300), deg))


def test_pointwise_sample_one_free_item_and_none(gpu_device):
    ptr, idx = S.dense_case()
    for seed in (12345, BIG_SEED):
        users, items, labels = _pointwise(gpu_device, 8, S.DENSE_I, ptr, idx, 3, seed)
        neg = labels == 0
        for name, free in (("free0", 0), ("free17", 17), ("free39", 39)):
            assert (items[neg & (users == S.DENSE_ROWS[name])] == free).all()
        full = neg & (users == S.DENSE_ROWS["full"])
        assert full.sum() == 3 * S.DENSE_I and (items[full] == 0).all()       # the documented (u, 0, 0) rows, the caller's to drop


def test_pointwise_sample_grid_stride(gpu_device):
    ptr, idx = S.sparse_case(600, 200, max_deg=104, seed=8)
    assert len(idx) * 71 > 8192 * 256
    _pointwise(gpu_device, 600, 200, ptr, idx, 70, BIG_SEED)


@pytest.mark.parametrize("sample", ["pointwise", "pairwise"])
def test_device_epoch_drops_the_rows_of_a_full_user(gpu_device, sample):
    ds = S.tiny_with_a_full_user(sample, gpu_device, "device")
    ep = ds.generate_epoch()
    tp, ti = ds.train_csr_sorted()
    deg = np.diff(tp)
    keys = set((np.repeat(np.arange(ds.n_users), deg) * ds.n_items + ti).tolist())
    if sample == "pointwise":
        u, i, l = (ep[k].cpu().numpy() for k in ("users", "items", "labels"))
        ratio = ds.config["negative_ratio"]
        assert len(u) == len(ti) * (ratio + 1) - ratio * ds.n_items and l.sum() == len(ti)
        assert not ((u == S.FULL_USER) & (l == 0)).any() and ((u == S.FULL_USER) & (l == 1)).sum() == ds.n_items
        assert i.min() >= 0 and i.max() < ds.n_items
        assert all(((a * ds.n_items + b) in keys) == (c == 1) for a, b, c in zip(u, i, l))
    else:
        u, p, n = (ep[k].cpu().numpy() for k in ("users", "positive_items", "negative_items"))
        assert len(u) > 0.9 * ds.traindataSize and S.FULL_USER not in u
        assert all((a * ds.n_items + b) in keys and (a * ds.n_items + c) not in keys for a, b, c in zip(u, p, n))


# ---------------------------------------------------------------- rk_coo_to_csr
def _coo_to_csr(dev, n_rows, row, col, val, nnz=None):
    nnz = len(row) if nnz is None else nnz
    m = max(nnz, 0)
    rowptr, c, v = _out(n_rows + 1, torch.int32, dev), _out(m, torch.int32, dev), _out(m, torch.float32, dev)
    ins = [_t(row, np.int64, dev), _t(col, np.int64, dev), _t(val, np.float32, dev)]
    rc = _lib.lib().rk_coo_to_csr(n_rows, nnz, *(_lib.ptr(t) for t in ins), _lib.ptr(rowptr), _lib.ptr(c), _lib.ptr(v), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, _host(rowptr, n_rows + 1), _host(c, m), _host(v, m)


def _coo_case(rng, n_rows, nnz):
    """sorted COO rows with rows 0, 1, the last two and a run in the middle empty (where n_rows allows), distinct values"""
    ok = np.ones(n_rows, dtype=bool)
    if n_rows > 8:
        ok[[0, 1, n_rows - 2, n_rows - 1]] = False
        ok[n_rows // 2: n_rows // 2 + 5] = False
    row = np.sort(rng.choice(np.nonzero(ok)[0], size=nnz)).astype(np.int64)
    return row, rng.integers(0, 2 ** 31 - 1, nnz).astype(np.int64), rng.random(nnz, dtype=np.float32)


def _coo_rowptr_restated(n_rows, row):
    """rowptr[r] = first e with row[e] >= r"""
    return np.searchsorted(row, np.arange(n_rows + 1), side="left")


@pytest.mark.parametrize("n_rows,nnz", [(1, 1), (1, 7), (255, 900), (256, 900), (257, 900), (1000, 3001), (1000, 0), (256, 0),
                                        (1000, 4096 * 256 + 3)])
def test_coo_to_csr(gpu_device, n_rows, nnz):
    row, col, val = _coo_case(np.random.default_rng(n_rows + nnz), n_rows, nnz)
    rc, (rowptr, t0), (c, t1), (v, t2) = _coo_to_csr(gpu_device, n_rows, row, col, val)
    assert rc == 0 and t0 and t1 and t2
    assert np.array_equal(rowptr, _coo_rowptr_restated(n_rows, row))
    assert rowptr[0] == 0 and rowptr[-1] == nnz
    assert np.array_equal(c, col.astype(np.int32)) and np.array_equal(v.view(np.uint32), val.view(np.uint32))


def test_coo_to_csr_refusals(gpu_device):
    row, col, val = _coo_case(np.random.default_rng(1), 100, 50)
    rc, (rowptr, t0), _, _ = _coo_to_csr(gpu_device, 100, row, col, val, nnz=-1)
    assert rc == EINVAL and t0 and (rowptr == SENT).all()
    # sizes are refused before anything is read or launched
    for n_rows, nnz in ((0, 0), (-1, 5), (100, 2 ** 31)):
        assert _lib.lib().rk_coo_to_csr(n_rows, nnz, None, None, None, None, None, None, _lib.stream_ptr()) == EINVAL, (n_rows, nnz)


# ---------------------------------------------------------------- rk_build_norm_adj
def _norm_adj_restated(U, I, ptr, idx):
    """float64 D^-1/2 A D^-1/2 of the bipartite graph in the entry point's layout: user rows (columns U + item, in the row's
    order), then item rows (users ascending); order[j] = the user-row entry that item-row entry j mirrors"""
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    E = len(idx)
    users = np.repeat(np.arange(U), np.diff(ptr))
    udeg, ideg = np.diff(ptr), np.bincount(idx, minlength=I)
    rowptr = np.concatenate([ptr, E + np.cumsum(ideg)])
    order = np.lexsort((users, idx))
    col = np.concatenate([U + idx, users[order]])
    val = 1.0 / np.sqrt(udeg[users].astype(np.float64) * ideg[idx].astype(np.float64))
    return rowptr, col, np.concatenate([val, val[order]]), order


def _norm_adj(dev, U, I, ptr, idx):
    E = len(idx)
    rowptr, col, val = _out(U + I + 1, torch.int32, dev), _out(2 * E, torch.int32, dev), _out(2 * E, torch.float32, dev)
    tmp = torch.empty(I + 1, dtype=torch.int32, device=dev)
    ins = [_t(ptr, np.int32, dev), _t(idx, np.int32, dev)]
    rc = _lib.lib().rk_build_norm_adj(U, I, _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val),
                                      _lib.ptr(tmp), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, _host(rowptr, U + I + 1), _host(col, 2 * E), _host(val, 2 * E)


def _check_norm_adj(dev, U, I, ptr, idx):
    E = len(idx)
    rc, (rowptr, t0), (col, t1), (val, t2) = _norm_adj(dev, U, I, ptr, idx)
    r_rowptr, r_col, r_val, order = _norm_adj_restated(U, I, ptr, idx)
    assert rc == 0 and t0 and t1 and t2, (U, I)
    assert np.array_equal(rowptr, r_rowptr) and np.array_equal(col, r_col), (U, I)
    rel = float(np.max(np.abs(val - r_val) / r_val)) if E else 0.0
    print(f"U={U} I={I} E={E}: largest relative error of a value {rel:.3e} (bound 4e-7)")
    assert np.allclose(val, r_val, rtol=4e-7, atol=0), (U, I, rel)
    # (u, U + i) and (U + i, u) hold the same two-factor fp32 product: the same bits
    assert np.array_equal(val[E:].view(np.uint32), val[:E][order].view(np.uint32)), (U, I)
    for i in np.nonzero(np.diff(rowptr[U:]) > 1)[0][:50]:
        row = col[rowptr[U + i]:rowptr[U + i + 1]]
        assert (np.diff(row) > 0).all(), (U, I, int(i))


def _adj_case(rng, U, I):
    """users of 0..12 items, some empty, one of 70 and one of 140 items where I allows; the first and the last item and a run
    in the middle are rated by nobody where I allows"""
    items = np.arange(I)
    if I > 8:
        items = np.setdiff1d(items, [0, I - 1, I // 2, I // 2 + 1])
    deg = np.minimum(rng.integers(0, 13, U), len(items))
    if U > 8:
        deg[[0, U // 3, U - 1]] = 0
        deg[1], deg[U - 2] = min(70, len(items)), min(140, len(items))
    return S.csr_of([rng.choice(items, size=k, replace=False) for k in deg])


@pytest.mark.parametrize("U,I", [(1, 1), (5, 3), (301, 1023), (301, 1024), (301, 1025), (77, 2053)])
def test_build_norm_adj(gpu_device, U, I):
    if U > 8:
        ptr, idx = _adj_case(np.random.default_rng(U + I), U, I)
        deg, ideg = np.diff(ptr), np.bincount(idx, minlength=I)
        assert deg.max() > 128 and ((deg > 64) & (deg <= 128)).any() and (deg == 0).any() and U % 4
        assert ideg[0] == 0 and ideg[-1] == 0 and ideg[I // 2] == 0
    else:
        ptr, idx = S.csr_of([np.arange(I)] * U)       # every user rated every item
    _check_norm_adj(gpu_device, U, I, ptr, idx)


def test_build_norm_adj_without_an_edge(gpu_device):
    U, I = 5, 7
    rc, (rowptr, t0), (col, t1), (val, t2) = _norm_adj(gpu_device, U, I, np.zeros(U + 1, dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert rc == 0 and t0 and t1 and t2 and not rowptr.any() and len(rowptr) == U + I + 1


def test_build_norm_adj_stride_loops(gpu_device):
    U, I, k = 3000, 1500, 700
    rng = np.random.default_rng(4)
    idx = np.sort(np.argsort(rng.random((U, I)), axis=1)[:, :k], axis=1).astype(np.int32).reshape(-1)
    ptr = (np.arange(U + 1) * k).astype(np.int32)
    assert 8192 * 256 < len(idx) < 8192 * 256 + 4096
    _check_norm_adj(gpu_device, U, I, ptr, idx)


# ---------------------------------------------------------------- rk_eligible_users
def _eligible(dev, ptr, idx, targets):
    U = len(ptr) - 1
    flags = torch.empty(U, dtype=torch.int32, device=dev)
    ids, count = _out(U, torch.int32, dev), _out(1, torch.int32, dev)
    ins = [_t(ptr, np.int32, dev), _t(idx, np.int32, dev), _t(targets, np.int32, dev)]
    rc = _lib.lib().rk_eligible_users(U, _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]) if len(targets) else None, len(targets),
                                      _lib.ptr(flags), _lib.ptr(ids), _lib.ptr(count), _lib.stream_ptr())
    torch.cuda.synchronize()
    (ids, t0), (count, t1) = _host(ids, U), _host(count, 1)
    ref = eligible_users(ptr, idx, np.asarray(targets, dtype=np.int32))
    assert rc == 0 and t0 and t1
    assert count[0] == len(ref) and np.array_equal(ids[:len(ref)], ref) and (ids[len(ref):] == SENT).all(), (U, list(targets))
    return ref


@pytest.mark.parametrize("U", [1, 63, 64, 65, 1023, 1024, 1025, 3000])
def test_eligible_users(gpu_device, U):
    I = 50
    rng = np.random.default_rng(U)
    deg = rng.integers(0, 9, U)
    deg[0] = 3
    ptr, idx = S.csr_of([rng.choice(I, size=k, replace=False) for k in deg])
    first, last = int(idx[0]), int(idx[ptr[1] - 1])        # the first and the last item of user 0's row
    for targets in ([], [first], [last], [49], [first, 0, 49, last]):
        ref = _eligible(gpu_device, ptr, idx, targets)
        assert (0 in ref) == (not set(targets) & set(idx[:3].tolist()))          # user 0's row is idx[:3]


def test_eligible_users_second_turn_of_the_stride_loop(gpu_device):
    U, I = 2048 * 256 + 100, 50
    rng = np.random.default_rng(2)
    deg = rng.integers(0, 4, U)
    cols = rng.integers(0, I - 9, U)[:, None] + np.cumsum(rng.integers(1, 4, (U, 3)), axis=1)     # three ascending distinct items
    assert cols.max() < I
    idx = cols[np.arange(3)[None, :] < deg[:, None]].astype(np.int32)     # the first deg[u] of three sorted distinct items
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ref = _eligible(gpu_device, ptr, idx, [3, 17, 48])
    assert 0 < len(ref) < U and ref[-1] > 2048 * 256


def test_eligible_users_nobody_and_everybody(gpu_device):
    U = 1500
    rng = np.random.default_rng(5)
    ptr, idx = S.csr_of([np.append(rng.choice(40, size=4, replace=False), 45) for _ in range(U)])
    assert len(_eligible(gpu_device, ptr, idx, [45])) == 0                # everyone holds the target
    assert len(_eligible(gpu_device, ptr, idx, [46, 47])) == U
    assert len(_eligible(gpu_device, ptr, idx, [])) == U
    assert len(_eligible(gpu_device, np.zeros(U + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), [])) == 0   # nobody has a row


# ---------------------------------------------------------------- rk_pred_shift
def _pred_shift_restated(before, after):
    """the kernel's order in float64: thread t adds (double)after[i] - (double)before[i] for i = t, t + 1024, ...; then the tree
    part[t] += part[t + o], o = 512 .. 1"""
    n = len(before)
    diff = after.astype(np.float64) - before.astype(np.float64)
    rows = np.zeros(((n + 1023) // 1024, 1024))
    rows.reshape(-1)[:n] = diff
    part = np.zeros(1024)
    for r in range(rows.shape[0]):
        m = min(1024, n - 1024 * r)
        part[:m] += rows[r, :m]
    o = 512
    while o > 0:
        part[:o] += part[o:2 * o]
        o >>= 1
    return np.array([part[0] / n if n > 0 else 0.0, part[0]])


def _pred_shift(dev, before, after):
    out = _out(2, torch.float64, dev)
    ins = [_t(before, np.float32, dev), _t(after, np.float32, dev)]
    rc = _lib.lib().rk_pred_shift(_lib.ptr(ins[0]), _lib.ptr(ins[1]), len(before), _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    got, tail = _host(out, 2)
    assert rc == 0 and tail
    return got


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 100003])
def test_pred_shift_bit_for_bit(gpu_device, n):
    rng = np.random.default_rng(n)
    cases = [(rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32))]
    # large values that cancel: +-1e6 in pairs, shuffled, over shifts of 1e-3; every partial sum rounds, so the order shows
    v = (1e6 * (1 + rng.random(n // 2))).astype(np.float32)
    cases.append(((1e-3 * rng.standard_normal(n)).astype(np.float32), rng.permutation(np.concatenate([v, -v, np.zeros(n % 2, dtype=np.float32)]))))
    for before, after in cases:
        got, ref = _pred_shift(gpu_device, before, after), _pred_shift_restated(before, after)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (n, got, ref)
    if n == 0:
        assert got[0] == 0.0 and got[1] == 0.0


# ---------------------------------------------------------------- rk_hit_counts
CUTOFFS = {1: [10], 4: [10, 20, 50, 100], 5: [100, 50, 20, 10, 5], 8: [100, 100, 50, 20, 20, 10, 1, 0]}


def _hit_counts_restated(rank, ks):
    return np.array([[(rank[:, t] < k).sum() for k in ks] for t in range(rank.shape[1])]).reshape(-1)


@pytest.mark.parametrize("n", [1, 16384, 16385, 64 * 16384 + 5])
def test_hit_counts_groups_of_cutoffs(gpu_device, n):
    rng = np.random.default_rng(n)
    for T in (1, 3):
        rank = rng.integers(0, 130, (n, T)).astype(np.int32)
        if n > 3:
            rank[rng.integers(0, n, 3)] = 2 ** 31 - 1
        rank_d = _t(rank, np.int32, gpu_device)
        for nk, ks in CUTOFFS.items():
            counts, ks_d = _out(T * nk, torch.int32, gpu_device), _t(ks, np.int32, gpu_device)
            rc = _lib.lib().rk_hit_counts(_lib.ptr(rank_d), n, T, _lib.ptr(ks_d), nk, _lib.ptr(counts), _lib.stream_ptr())
            torch.cuda.synchronize()
            got, tail = _host(counts, T * nk)
            ref = _hit_counts_restated(rank, ks)
            assert rc == 0 and tail and np.array_equal(got, ref), (n, T, ks, got, ref)


# ---------------------------------------------------------------- rk_pair_scores
def _pair_scores(dev, tabs, users, items, mean, dropout, seed, bias=(True, True)):
    utab, itab, ub, ib = tabs
    n = len(users)
    out = _out(n, torch.float32, dev)
    ins = [_t(utab, np.float32, dev), _t(itab, np.float32, dev), _t(ub, np.float32, dev), _t(ib, np.float32, dev),
           _t(users, np.int64, dev), _t(items, np.int64, dev)]
    rc = _lib.lib().rk_pair_scores(utab.shape[1], _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]) if bias[0] else None,
                                   _lib.ptr(ins[3]) if bias[1] else None, mean, _lib.ptr(ins[4]), _lib.ptr(ins[5]), n, _lib.ptr(out),
                                   dropout, seed, _lib.stream_ptr())
    torch.cuda.synchronize()
    return (rc,) + _host(out, n)


def _pair_scores_restated(tabs, users, items, mean, biased):
    """-> the float64 scores and S = sum |u_k i_k| + |ub| + |ib| + |mean|"""
    u, i, ub, ib = (t.astype(np.float64) for t in tabs)
    prod = u[users] * i[items]
    if not biased:
        return prod.sum(1), np.abs(prod).sum(1)
    return prod.sum(1) + ub[users] + ib[items] + mean, np.abs(prod).sum(1) + np.abs(ub[users]) + np.abs(ib[items]) + abs(mean)


@pytest.mark.parametrize("d", [1, 63, 64, 65, 130, 256])
def test_pair_scores(gpu_device, d):
    rng = np.random.default_rng(d)
    nu, ni = 37, 53
    tabs = (rng.standard_normal((nu, d)).astype(np.float32), rng.standard_normal((ni, d)).astype(np.float32),
            rng.standard_normal(nu).astype(np.float32), rng.standard_normal(ni).astype(np.float32))
    mean = float(np.float32(3.53))
    m = math.ceil(d / 64) + 6 + 3 + 2
    worst = 0.0
    for n in (1, 3, 4, 5, 4096 * 4 + 9):
        users, items = rng.integers(0, nu, n), rng.integers(0, ni, n)
        if n >= 3:
            users[1], items[1] = users[0], items[0]          # a repeated pair
            users[-1], items[-1] = nu - 1, ni - 1            # the last row of both tables
        for biased in (True, False):
            ref, S_ = _pair_scores_restated(tabs, users, items, mean, biased)
            bound = m * 2.0 ** -24 * S_
            rc, plain, tail = _pair_scores(gpu_device, tabs, users, items, mean, 0.0, 0, bias=(biased, biased))
            worst = max(worst, float(np.max(np.abs(plain - ref) / bound)))
            assert rc == 0 and tail and (np.abs(plain - ref) <= bound).all(), (d, n, biased)
            if n >= 3:
                assert plain[0] == plain[1]
            for p, seed in ((0.25, 99), (0.9, BIG_SEED)):
                p32 = float(np.float32(p))
                keep = _drop_keep(seed, n, 1.0 - p32)
                scale32 = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
                rc, got, tail = _pair_scores(gpu_device, tabs, users, items, mean, p32, seed, bias=(biased, biased))
                assert rc == 0 and tail
                assert np.array_equal(got != 0, keep) and (plain != 0).all(), (d, n, biased, p)     # the mask, element for element
                assert (np.abs(got[keep] - ref[keep] / (1.0 - p32)) <= bound[keep] / (1.0 - p32)).all(), (d, n, biased, p)
                assert np.array_equal(got[keep], plain[keep] * scale32), (d, n, biased, p)
    print(f"d={d}: largest error / bound {worst:.3f} (m = {m})")


def test_pair_scores_refusals(gpu_device):
    rng = np.random.default_rng(0)
    tabs = (rng.standard_normal((4, 8)).astype(np.float32), rng.standard_normal((4, 8)).astype(np.float32),
            np.ones(4, dtype=np.float32), np.ones(4, dtype=np.float32))
    users = items = np.arange(4)
    for kw in ({"bias": (True, False)}, {"bias": (False, True)}):
        rc, out, tail = _pair_scores(gpu_device, tabs, users, items, 0.0, 0.0, 0, **kw)
        assert rc == EINVAL and tail and (out == SENT).all(), kw
    for p in (1.0, 1.5, -0.1, float("nan")):
        rc, out, tail = _pair_scores(gpu_device, tabs, users, items, 0.0, p, 0)
        assert rc == EINVAL and tail and (out == SENT).all(), p
