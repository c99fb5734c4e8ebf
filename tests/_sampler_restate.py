"""numpy restatement of recad_amd/csrc/sampler.hip, vectorised over the draw index t: rnd, bounded, lower_bound, rth_free_item,
bpr_sample_kernel and pointwise_sample_kernel, step for step and in uint64 wrap-around arithmetic, so that a device run can be
compared element for element.  The binary searches are the kernels' own loops (same mid, same comparison), run on every still
unfinished draw at once.  Test infrastructure only."""
import numpy as np

from ._drop_restate import _mix64

_C = np.uint64(0xD1342543DE82EF95)
_32 = np.uint64(32)


def rnd(seed, draw, k):
    """rnd(seed, draw, k) of sampler.hip for an array of draw indices"""
    with np.errstate(over="ignore"):
        return _mix64(_mix64(np.uint64(seed) ^ (np.asarray(draw, dtype=np.uint64) * _C)) + np.uint64(k))


def bounded(r, n):
    """((r >> 32) * n) >> 32: both factors are below 2^32, the product does not wrap"""
    return (((np.asarray(r, dtype=np.uint64) >> _32) * np.asarray(n, dtype=np.uint64)) >> _32).astype(np.int64)


def _at(a, p):
    """a[p] where p is inside a, 0 elsewhere (the kernels never read those: every such read is guarded)"""
    p = np.asarray(p, dtype=np.int64)
    ok = (p >= 0) & (p < len(a))
    out = np.zeros(p.shape, dtype=np.int64)
    out[ok] = a[p[ok]]
    return out


def lower_bound(a, lo, hi, x):
    """first p in [lo, hi) with a[p] >= x, else hi; lo, hi, x arrays of one length"""
    lo, hi, x = (np.array(v, dtype=np.int64) for v in (lo, hi, x))
    while True:
        act = lo < hi
        if not act.any():
            return lo
        mid = (lo + hi) >> 1
        less = act & (_at(a, mid) < x)
        lo = np.where(less, mid + 1, lo)
        hi = np.where(act & ~less, mid, hi)


def rth_free_item(idx, b, e, r):
    """r-th (0-based) item not in the sorted row idx[b:e); b, e, r arrays of one length"""
    b, e, r = (np.array(v, dtype=np.int64) for v in (b, e, r))
    lo, hi = np.zeros_like(b), e - b
    while True:
        act = lo < hi
        if not act.any():
            return r + lo
        mid = (lo + hi) >> 1
        le = act & (_at(idx, b + mid) - mid <= r)
        lo = np.where(le, mid + 1, lo)
        hi = np.where(act & ~le, mid, hi)


def bpr_sample(n_users, n_items, ptr, idx, n_draws, seed):
    """-> users, pos, neg (int64[n_draws]), valid (int32[n_draws]) as bpr_sample_kernel writes them, and fallback (bool[n_draws]):
    the draws whose 64 rejection attempts all clashed and that took the rth_free_item draw"""
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    t = np.arange(n_draws, dtype=np.uint64)
    users = bounded(rnd(seed, t, 0), n_users)
    b, e = ptr[users], ptr[users + 1]
    deg = e - b
    live = np.nonzero(~((deg == 0) | (deg >= n_items)))[0]
    pos, neg = np.zeros(n_draws, dtype=np.int64), np.zeros(n_draws, dtype=np.int64)
    valid = np.zeros(n_draws, dtype=np.int32)
    fallback = np.zeros(n_draws, dtype=bool)
    valid[live] = 1
    pos[live] = _at(idx, b[live] + bounded(rnd(seed, t[live], 1), deg[live]))
    todo = live
    for k in range(2, 66):
        if not len(todo):
            break
        ng = bounded(rnd(seed, t[todo], k), n_items)
        p = lower_bound(idx, b[todo], e[todo], ng)
        ok = ~((p < e[todo]) & (_at(idx, p) == ng))
        neg[todo] = ng
        todo = todo[~ok]
    if len(todo):
        r = bounded(rnd(seed, t[todo], 66), n_items - deg[todo])
        neg[todo] = rth_free_item(idx, b[todo], e[todo], r)
        fallback[todo] = True
    return users, pos, neg, valid, fallback


def edge_user(n_users, ptr, e):
    """the pointwise kernel's search: last u in [0, n_users] with ptr[u] <= e"""
    e = np.asarray(e, dtype=np.int64)
    lo, hi = np.zeros_like(e), np.full_like(e, n_users)
    while True:
        act = lo < hi
        if not act.any():
            return lo
        mid = (lo + hi + 1) >> 1
        le = act & (ptr[mid] <= e)
        lo = np.where(le, mid, lo)
        hi = np.where(act & ~le, mid - 1, hi)


def pointwise_sample(n_users, n_items, ptr, idx, ratio, seed):
    """-> users, items, labels (int64[E * (ratio + 1)]) as pointwise_sample_kernel writes them; a user without a free item gets
    (u, 0, 0) in its negative rows"""
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    total = int(ptr[n_users]) * (ratio + 1)
    t = np.arange(total, dtype=np.int64)
    e, k = t // (ratio + 1), t % (ratio + 1)
    users = edge_user(n_users, ptr, e)
    b, en = ptr[users], ptr[users + 1]
    free = n_items - (en - b)
    items = np.zeros(total, dtype=np.int64)
    labels = (k == 0).astype(np.int64)
    items[k == 0] = idx[e[k == 0]]
    ng = np.nonzero((k != 0) & (free > 0))[0]
    r = bounded(rnd(seed, ng.astype(np.uint64), 0), free[ng])
    items[ng] = rth_free_item(idx, b[ng], en[ng], r)
    return users, items, labels


# ---------------------------------------------------------------- the graphs the sampler tests share
def csr_of(rows):
    """-> ptr, idx (int32) of a list of item lists, each row sorted and distinct"""
    rows = [np.unique(np.asarray(r, dtype=np.int32)) for r in rows]
    ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, np.concatenate(rows + [np.zeros(0, dtype=np.int32)]).astype(np.int32)


def sparse_case(n_users=300, n_items=200, max_deg=30, seed=7):
    """rows of 0..max_deg items; users 0, 1, 2, a middle one and the last two are empty"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, max_deg + 1, n_users)
    deg[[0, 1, 2, n_users // 2, n_users - 2, n_users - 1]] = 0
    return csr_of([rng.choice(n_items, size=k, replace=False) for k in deg])


DENSE_I = 40
DENSE_ROWS = {"free0": 0, "free17": 1, "free39": 2, "deg38": 3, "full": 4, "empty": 5, "deg1": 6, "deg20": 7}


def dense_case():
    """U = 8, I = 40: three rows of 39 items (free item 0, 17, 39), one of 38, the full row, an empty row, 1 item, 20 items"""
    every = np.arange(DENSE_I)
    return csr_of([np.delete(every, 0), np.delete(every, 17), np.delete(every, 39), np.delete(every, [5, 30]), every, [], [13],
                   every[::2]])


FULL_USER = 5


def tiny_with_a_full_user(sample, device, sampler):
    """the `tiny` synthetic set with user 5 given every item in train"""
    from recad_amd import dataset, synth
    d = synth.make("tiny")
    ptr, idx = (np.asarray(a) for a in d["train"])
    rows = [idx[ptr[u]:ptr[u + 1]] for u in range(len(ptr) - 1)]
    rows[FULL_USER] = np.arange(d["n_items"], dtype=idx.dtype)
    train = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(ptr.dtype), np.concatenate(rows))
    return dataset.from_config("implicit", "tiny", train_csr=train, valid_csr=d["valid"], test_csr=d["test"], need_graph=False,
                               device=device, sample=sample, graph_source="train", sampler=sampler, seed=3)
