"""GPU tests of the CatchSyncSelectUsers kernels one entry point at a time (csrc/catchsync.hip) against the numpy restatement
of the definition (tests/_catchsync_restate.py).  Every entry runs from inputs the test owns; everything is compared word for
word: no tolerance, no excluded case.  Every output buffer is pre-filled with a sentinel (floats: NaN) and carries a
64-element margin that must stay as it was."""
import numpy as np
import pytest
import torch

from recad_amd import _lib
from tests import _catchsync_restate as R

pytestmark = pytest.mark.gpu
MARGIN, SENTINEL = 64, -777
EINVAL = -22


class Out:
    """A device buffer of n elements followed by MARGIN more, all NaN (floats) or SENTINEL (ints)."""

    def __init__(self, n, dtype, dev):
        self.n, self.fp = int(n), dtype.is_floating_point
        self.full = torch.full((self.n + MARGIN,), float("nan") if self.fp else SENTINEL, dtype=dtype, device=dev)

    def host(self):
        tail = self.full[self.n:].cpu().numpy()
        assert (np.isnan(tail).all() if self.fp else (tail == SENTINEL).all()), "the kernel wrote past the end of its output"
        return self.full[: self.n].cpu().numpy()

    def untouched(self):
        a = self.full.cpu().numpy()
        return bool(np.isnan(a).all() if self.fp else (a == SENTINEL).all())


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


# ------------------------------------------------------------------------------------------------------------ rk_cs_features
COLUMN_LENGTHS = (0, 1, 63, 64, 65, 257)


@pytest.mark.parametrize("U", [1, 5, 70, 300])
def test_features(gpu_device, U):
    """Columns of 0, 1, 63..65 and 257 users (capped at U) in turn, column 0 with every user; then the same graph with the
    first, the middle and the last row emptied."""
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(gpu_device)
    rng = np.random.default_rng(U)
    for I in (1, 2, 63, 64, 65, 200, 257):
        A = np.zeros((U, I), dtype=bool)
        for j in range(I):
            A[rng.permutation(U)[: min(COLUMN_LENGTHS[(j + 5) % 6], U)], j] = True
        A[:, 0] = True
        for empty_rows in (False, True):
            if empty_rows:
                A[[0, U // 2, U - 1]] = False
            ptr, idx = _csr_of(A)
            colptr, crow = _transpose(ptr, idx, I)
            deg, reach = Out(I, torch.int32, gpu_device), Out(I, torch.int32, gpu_device)
            d = [_dev(a, gpu_device) for a in (ptr, colptr, crow)]
            assert L.rk_cs_features(U, I, P(d[0]), P(d[1]), P(d[2]), P(deg.full), P(reach.full), s) == 0
            torch.cuda.synchronize()
            want_deg, want_reach = R.features(ptr, idx, I)
            assert np.array_equal(deg.host(), want_deg) and np.array_equal(reach.host(), want_reach), (U, I, empty_rows)
            if not empty_rows:
                assert want_deg[0] == U and want_reach[0] == len(idx)


def test_features_refusals(gpu_device):
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(gpu_device)
    out = Out(4, torch.int32, gpu_device)
    z = torch.zeros(8, dtype=torch.int32, device=gpu_device)
    assert L.rk_cs_features(0, 4, P(z), P(z), P(z), P(out.full), P(out.full), s) == EINVAL
    assert L.rk_cs_features(4, 0, P(z), P(z), P(z), P(out.full), P(out.full), s) == EINVAL
    assert L.rk_cs_features(4, 4, P(z), None, P(z), P(out.full), P(out.full), s) == EINVAL
    torch.cuda.synchronize()
    assert out.untouched()


# --------------------------------------------------------------------------------------------------------------- rk_cs_cells
def _cells(dev, deg, reach, s):
    I = len(deg)
    o = {"cell_of": Out(I, torch.int32, dev), "cell_count": Out(_lib.RK_CS_MAX_CELLS, torch.int32, dev),
         "info": Out(4, torch.int64, dev), "status": Out(2, torch.int32, dev)}
    L, P = _lib.lib(), _lib.ptr
    d = [_dev(np.asarray(a, dtype=np.int32), dev) for a in (deg, reach)]
    rc = L.rk_cs_cells(I, P(d[0]), P(d[1]), s, P(o["cell_of"].full), P(o["cell_count"].full), P(o["info"].full), P(o["status"].full),
                       _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, o


def _check_cells(dev, deg, reach, s):
    want = R.cells(deg, reach, s)
    rc, o = _cells(dev, deg, reach, s)
    if isinstance(want[0], str):
        assert rc == EINVAL and o["status"].host().tolist() == [want[1], want[2]]
        assert o["cell_of"].untouched() and o["cell_count"].untouched() and o["info"].untouched(), "outputs must be untouched after a refusal"
        msg = _lib.lib().rk_last_error().decode()
        assert f"rule {want[1]}" in msg and f"item {want[2]}" in msg
        return want
    assert rc == 0 and o["status"].host().tolist() == [0, -1]
    assert np.array_equal(o["cell_of"].host(), want[0])
    assert np.array_equal(o["cell_count"].host(), want[1])
    assert o["info"].host().tolist() == list(want[2])
    return want


def _boundaries(s):
    """Every x = 2^e (2^s + m) / 2^s that is an integer, e <= 30, with its two neighbours, inside [1, 2^31 - 1]."""
    xs = {1, 2, 3, 2 ** 31 - 1}
    for e in range(31):
        for m in range(1 << s):
            num = (1 << e) * ((1 << s) + m)
            if num % (1 << s) == 0:
                xs.update((num >> s) + t for t in (-1, 0, 1))
    return np.array(sorted(x for x in xs if 1 <= x <= 2 ** 31 - 1), dtype=np.int64)


@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_cells_bucket_boundaries(gpu_device, s):
    """Every boundary value once as deg_item and once (seven places on) as reach; unrated items first, in the middle, last."""
    x = _boundaries(s)
    deg, reach = x.copy(), np.roll(x, 7)
    mid = len(x) // 2
    deg = np.concatenate([[0], deg[:mid], [0, 0], deg[mid:], [0]])
    reach = np.concatenate([[0], reach[:mid], [0, 5], reach[mid:], [0]])       # an unrated item's reach is not read
    cell_of, _, info = _check_cells(gpu_device, deg, reach, s)
    assert cell_of[0] == cell_of[-1] == cell_of[mid + 1] == cell_of[mid + 2] == -1 and info[1] == len(x)
    assert info[0] > 31 * (1 << s) // 2                                         # the grid really is finer with more bits


def _rep(b):
    """A value whose bucket at s = 3 is b + 24 (e = 3 + b // 8, m = b % 8)."""
    return (8 + b % 8) << (b // 8)


def _m_cells(M, rng):
    """Items with exactly M distinct keys at s = 3, some keys repeated, in shuffled order."""
    pairs = [(c // 128, c % 128) for c in range(M)]
    extra = [pairs[int(j)] for j in rng.integers(0, M, size=min(M, 300))] if M != 64 else []       # M = 64: all cells equal
    items = np.array(pairs + extra)
    items = items[rng.permutation(len(items))]
    return np.array([_rep(a) for a in items[:, 0]]), np.array([_rep(b) for b in items[:, 1]])


@pytest.mark.parametrize("M", [1, 2, 64, 65, 8192])
def test_cells_counts(gpu_device, M):
    rng = np.random.default_rng(M)
    deg, reach = _m_cells(M, rng)
    _, _, info = _check_cells(gpu_device, deg, reach, 3)
    assert info[0] == M and (info[3] == 1 if M in (1, 64) else M == 2 or info[3] == 0)
    first, again = _cells(gpu_device, deg, reach, 3)[1], _cells(gpu_device, deg, reach, 3)[1]
    assert all(np.array_equal(again[k].host(), first[k].host()) for k in again), "the same call twice gives the same words"


def test_cells_single_item_and_no_rated_item(gpu_device):
    assert _check_cells(gpu_device, [4], [9], 1)[2] == (1, 1, 1, 1)
    assert _check_cells(gpu_device, [0], [0], 1)[2] == (0, 0, 0, 1)
    assert _check_cells(gpu_device, [0, 0, 0], [0, 0, 0], 2)[2][0] == 0


def test_cells_refusals(gpu_device):
    rng = np.random.default_rng(3)
    deg, reach = _m_cells(8192, rng)
    # one more key, above every other, at item 100 and again at the end: the lowest item of the 8193rd cell is reported
    big = 2 ** 31 - 1
    deg2 = np.concatenate([deg[:100], [big], deg[100:], [big]])
    reach2 = np.concatenate([reach[:100], [big], reach[100:], [big]])
    assert _check_cells(gpu_device, deg2, reach2, 3) == ("refused", R.TOO_MANY_CELLS, 100)
    for name, (d, r) in {"deg": (-1, 5), "reach": (3, -2), "zero reach": (3, 0)}.items():
        dd, rr = deg[:500].copy(), reach[:500].copy()
        dd[[123, 400]], rr[[123, 400]] = d, r
        assert _check_cells(gpu_device, dd, rr, 3) == ("refused", R.BAD_FEATURE, 123), name
    # a bad feature before the overflowing item wins; after it, the overflowing item does
    deg2[50] = -4
    assert _check_cells(gpu_device, deg2, reach2, 3)[1:] == (R.BAD_FEATURE, 50)
    deg2[50], deg2[-1] = deg[50], -4                                   # the last item repeats item 100's key: still 8193 cells
    assert _check_cells(gpu_device, deg2, reach2, 3)[1:] == (R.TOO_MANY_CELLS, 100)
    # argument refusals: nothing launched, nothing written
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(gpu_device)
    z = torch.ones(8, dtype=torch.int32, device=gpu_device)
    o = [Out(8, torch.int32, gpu_device), Out(_lib.RK_CS_MAX_CELLS, torch.int32, gpu_device), Out(4, torch.int64, gpu_device),
         Out(2, torch.int32, gpu_device)]
    for I, bits in ((8, -1), (8, 4), (0, 1), (_lib.RK_CS_MAX_ITEMS, 1)):
        assert L.rk_cs_cells(I, P(z), P(z), bits, P(o[0].full), P(o[1].full), P(o[2].full), P(o[3].full), s) == EINVAL
    assert L.rk_cs_cells(8, P(z), None, 1, P(o[0].full), P(o[1].full), P(o[2].full), P(o[3].full), s) == EINVAL
    torch.cuda.synchronize()
    assert all(x.untouched() for x in o)


# ----------------------------------------------------------------------------------------------------------- rk_cs_user_sums
ROW_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 600, 1100)      # 512: the automatic form's threshold
N_ITEMS = 2400


def _sums_case(M, rng):
    """cell_of over 2400 items: 0..1199 random cells with -1, M, M + 5 and 2^31 - 1 sprinkled in (skipped), 1200..1799 all in
    one cell, 1800..2399 cell i - 1800 (mod M); cell_count up to 2^26 so that back_num passes 2^31."""
    cell_of = np.empty(N_ITEMS, dtype=np.int32)
    cell_of[:1200] = rng.integers(0, M, size=1200)
    cell_of[rng.permutation(1200)[:90]] = np.repeat([-1, M, M + 5, 2 ** 31 - 1, -2 ** 31], 18)
    cell_of[1200:1800] = min(3, M - 1)
    cell_of[1800:] = np.arange(600) % M
    cell_count = np.zeros(_lib.RK_CS_MAX_CELLS, dtype=np.int32)
    cell_count[:M] = rng.integers(1, 2 ** 26, size=M)
    rows = [np.sort(rng.permutation(1200)[:n]) for n in ROW_LENGTHS]
    rows.append(np.arange(1200, 1800))                                 # wholly in one cell: pair_num = d^2
    rows.append(np.arange(1800, 1800 + min(M, 600)))                   # all-distinct cells: pair_num = d
    rows.append(np.arange(0, N_ITEMS, 2))                              # 1 200 items of every kind
    rows = [rows[i] for i in rng.permutation(len(rows))] + [np.zeros(0, dtype=np.int64)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return ptr, np.concatenate(rows).astype(np.int32), cell_of, cell_count


def _user_sums(dev, ptr, idx, cell_of, cell_count, M, form, order):
    U = len(ptr) - 1
    pair, back = Out(U, torch.int64, dev), Out(U, torch.int64, dev)
    L, P = _lib.lib(), _lib.ptr
    d = [_dev(a, dev) for a in (ptr, idx, cell_of, cell_count)]
    o = None if order is None else _dev(np.asarray(order, dtype=np.int32), dev)
    rc = L.rk_cs_user_sums(U, P(d[0]), P(d[1]), P(d[2]), P(d[3]), M, form, P(o), P(pair.full), P(back.full), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, pair, back


@pytest.mark.parametrize("M", [1, 2, 64, 65, 1024, 1025, 8192])
def test_user_sums(gpu_device, M):
    rng = np.random.default_rng(100 + M)
    ptr, idx, cell_of, cell_count = _sums_case(M, rng)
    U = len(ptr) - 1
    want_pair, want_back = R.user_sums(ptr, idx, cell_of, cell_count, M)
    d = np.diff(ptr)
    one, distinct = [u for u in range(U) if d[u] == 600 and idx[ptr[u]] == 1200], [u for u in range(U) if d[u] and idx[ptr[u]] == 1800]
    assert want_pair[one[0]] == 600 * 600 and want_pair[distinct[0]] == d[distinct[0]] == min(M, 600) and want_back.max() > 2 ** 31
    skipped = rng.permutation(U)[:2]
    random_order = rng.permutation(U)
    random_order[np.isin(random_order, skipped)] = [U + 5, -1]         # two entries out of range: those users are never written
    orders = {"null": None, "identity": np.arange(U), "reversed": np.arange(U)[::-1], "random": random_order}
    for form in (1, 2, 0):
        for name, order in orders.items():
            rc, pair, back = _user_sums(gpu_device, ptr, idx, cell_of, cell_count, M, form, order)
            wp, wb = want_pair.copy(), want_back.copy()
            if name == "random":
                wp[skipped] = wb[skipped] = SENTINEL
            assert rc == 0 and np.array_equal(pair.host(), wp) and np.array_equal(back.host(), wb), (M, form, name)


@pytest.mark.parametrize("M", [7, 8192])
def test_user_sums_many_users_per_workgroup(gpu_device, M):
    """300 users: a workgroup of the wave form serves 32 entries of `order` (10 workgroups, 8 users in turn on each wave's
    slice), one of the workgroup form 8 (38 workgroups): a histogram word left over from the previous user would add to the
    next user's pair_num.  Rows overlap heavily (60 items, 7 cells) so that every user touches every cell."""
    rng = np.random.default_rng(M)
    I = 60 if M == 7 else 9000
    rows = [np.sort(rng.permutation(I)[: int(n)]) for n in rng.integers(1, 50, size=300)]
    rows[17] = np.arange(I)[:600]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    idx = np.concatenate(rows).astype(np.int32)
    cell_of = rng.integers(0, M, size=I).astype(np.int32)
    cell_count = np.zeros(_lib.RK_CS_MAX_CELLS, dtype=np.int32)
    cell_count[:M] = np.bincount(cell_of, minlength=M)
    want_pair, want_back = R.user_sums(ptr, idx, cell_of, cell_count, M)
    for form in (1, 2, 0):
        for order in (None, rng.permutation(300)):
            rc, pair, back = _user_sums(gpu_device, ptr, idx, cell_of, cell_count, M, form, order)
            assert rc == 0 and np.array_equal(pair.host(), want_pair) and np.array_equal(back.host(), want_back), (form, order is None)


def test_user_sums_refusals(gpu_device):
    ptr, idx = np.array([0, 2, 3], dtype=np.int32), np.array([0, 1, 1], dtype=np.int32)
    cell_of, cell_count = np.zeros(2, dtype=np.int32), np.ones(_lib.RK_CS_MAX_CELLS, dtype=np.int32)
    for M, form in ((0, 0), (-1, 1), (_lib.RK_CS_MAX_CELLS + 1, 0), (1, 3), (1, -1)):
        rc, pair, back = _user_sums(gpu_device, ptr, idx, cell_of, cell_count, M, form, None)
        assert rc == EINVAL and pair.untouched() and back.untouched(), (M, form)
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(gpu_device)
    z = torch.zeros(8, dtype=torch.int32, device=gpu_device)
    out = Out(2, torch.int64, gpu_device)
    assert L.rk_cs_user_sums(0, P(z), P(z), P(z), P(z), 1, 0, None, P(out.full), P(out.full), s) == EINVAL
    assert L.rk_cs_user_sums(2, P(z), P(z), None, P(z), 1, 0, None, P(out.full), P(out.full), s) == EINVAL
    assert L.rk_cs_user_sums(2, P(z), P(z), P(z), P(z), 1, 0, None, P(out.full), None, s) == EINVAL
    torch.cuda.synchronize()
    assert out.untouched()


# -------------------------------------------------------------------------------------------------------------- rk_cs_scores
def _scores(dev, ptr, pair, back, info, mode, min_items):
    U = len(ptr) - 1
    out = Out(U, torch.float32, dev)
    L, P = _lib.lib(), _lib.ptr
    d = [_dev(np.asarray(ptr, dtype=np.int32), dev)] + [_dev(np.asarray(a, dtype=np.int64), dev) for a in (pair, back, info)]
    rc = L.rk_cs_scores(U, P(d[0]), P(d[1]), P(d[2]), P(d[3]), mode, min_items, P(out.full), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, out


def _score_inputs(rng, min_items, M, N):
    """Row lengths around min_items, 2 and long ones; for each a few feasible (pair_num, back_num): d <= pair <= d^2,
    d <= back <= d * N, the extremes included."""
    lengths = [0, 1, 2, 3, min_items - 1, min_items, min_items + 1, 36, 37, 600, 1100, 40000]
    d = np.repeat(lengths, 6)
    lo = np.maximum(d, 0).astype(np.int64)
    frac = np.tile([0.0, 1.0, 0.5, 0.013, 0.77, 0.31], len(lengths))
    pair = lo + np.floor(frac * (lo * lo - lo)).astype(np.int64)
    back = lo + np.floor(np.roll(frac, 1) * (lo * N - lo)).astype(np.int64)
    return np.concatenate([[0], np.cumsum(d)]), pair, back


@pytest.mark.parametrize("all_equal", [0, 1])
@pytest.mark.parametrize("min_items", [2, 20, 30])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scores(gpu_device, mode, min_items, all_equal):
    rng = np.random.default_rng(mode * 100 + min_items)
    M, N = (38, 3702) if not all_equal else (64, 64 * 57)
    SB = 1198696 if not all_equal else 64 * 57 * 57
    info = (M, N, SB, all_equal)
    ptr, pair, back = _score_inputs(rng, min_items, M, N)
    rc, out = _scores(gpu_device, ptr, pair, back, info, mode, min_items)
    want = R.scores(ptr, pair, back, info, R.MODES[mode], min_items)
    assert rc == 0 and np.array_equal(out.host().view(np.uint32), want.view(np.uint32))
    d = np.diff(ptr)
    assert np.all(want[d < min_items] == np.float32(-1))
    assert mode == 2 or np.all(want[d >= min_items] >= 0), "sync and normality of an eligible user are not negative"
    if mode == 0:
        assert want[(d >= min_items) & (pair == d * d)].tolist() == [1.0] * int(((d >= min_items) & (pair == d * d)).sum())


def test_scores_single_cell_and_large_integers(gpu_device):
    """M = 1 (s_min = 1 / M = 1, the residual of a user wholly in that cell is 0) and sums near 2^52."""
    ptr = np.array([0, 50, 50 + 2 ** 20])
    info = (1, 2 ** 25, 2 ** 50, 1)
    pair, back = np.array([2500, 2 ** 40]), np.array([50 * 2 ** 25, 2 ** 45])
    for mode in (0, 1, 2):
        rc, out = _scores(gpu_device, ptr, pair, back, info, mode, 2)
        want = R.scores(ptr, pair, back, info, R.MODES[mode], 2)
        assert rc == 0 and np.array_equal(out.host().view(np.uint32), want.view(np.uint32))
        assert want.tolist() == [[1.0, 1.0], [1.0, 1.0], [0.0, 0.0]][mode]


def test_scores_refusals(gpu_device):
    ptr, pair, back, info = np.array([0, 30, 60]), np.array([100, 100]), np.array([100, 100]), (4, 100, 2600, 0)
    for mode, min_items in ((-1, 20), (3, 20), (0, 1), (1, 0), (2, -5)):
        rc, out = _scores(gpu_device, ptr, pair, back, info, mode, min_items)
        assert rc == EINVAL and out.untouched(), (mode, min_items)
    L, P, s = _lib.lib(), _lib.ptr, _lib.stream_ptr(gpu_device)
    z, z64 = torch.zeros(8, dtype=torch.int32, device=gpu_device), torch.zeros(8, dtype=torch.int64, device=gpu_device)
    out = Out(2, torch.float32, gpu_device)
    assert L.rk_cs_scores(0, P(z), P(z64), P(z64), P(z64), 0, 20, P(out.full), s) == EINVAL
    assert L.rk_cs_scores(2, P(z), P(z64), None, P(z64), 0, 20, P(out.full), s) == EINVAL
    assert L.rk_cs_scores(2, P(z), P(z64), P(z64), P(z64), 0, 20, None, s) == EINVAL
    torch.cuda.synchronize()
    assert out.untouched()
