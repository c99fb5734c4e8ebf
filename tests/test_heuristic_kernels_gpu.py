"""GPU tests of csrc/heuristic.hip, one entry point at a time against the float64 restatement (tests/_heuristic_restate.py):
rk_heur_item_stats, rk_heur_popular, rk_heur_generate in its replay form (exact) and with its own draws (structure exact,
columns equal to the restated integer RNG, values in distribution), and every refusal.

Bounds.  Counts, popular ids and every profile are compared exactly.  A mean of `count` float64 terms summed in any order is
within count * 2^-52 * max|rating| of the exact one (R.stat_bound); the device's per-item sums are float64 atomics, its
global sums a fixed tree, the restatement's are numpy's -- three orders, one bound.  The two statistical checks are derived
where they stand."""
import ctypes as C

import numpy as np
import pytest
import torch

from recad_amd import _lib

from . import _heuristic_restate as R

pytestmark = pytest.mark.gpu
EINVAL = -22
ITEMS = (1, 63, 64, 65, 257, 1025)
USERS = (1, 3, 300)


def _t(a, dtype, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def dev_stats(dev, I, col, val):
    col_t, val_t = _t(col, np.int32, dev), _t(val, np.float32, dev)
    cnt = torch.full((I,), -7, dtype=torch.int32, device=dev)
    mean = torch.full((I,), -7.0, dtype=torch.float64, device=dev)
    glob = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    nr = torch.full((1,), -7, dtype=torch.int32, device=dev)
    n = len(col)
    rc = _lib.lib().rk_heur_item_stats(I, n, _lib.ptr(col_t) if n else None, _lib.ptr(val_t) if n else None, _lib.ptr(cnt), _lib.ptr(mean),
                                       _lib.ptr(glob), _lib.ptr(nr), _lib.stream_ptr(dev))
    _lib.check(rc, "rk_heur_item_stats")
    return cnt.cpu().numpy(), mean.cpu().numpy(), glob.cpu().numpy(), int(nr.cpu().numpy()[0])


def craft_ratings(U, I, seed, dense=False):
    """(col, val) of a U-user rating CSR over I items with non-integer ratings: item 0 rated by everybody (one long item row),
    item 1 by user 0 alone (a single rating), the last item by nobody (when I > 2), the rest at random."""
    rng = np.random.default_rng(seed)
    cols = []
    for u in range(U):
        if dense:
            c = np.arange(I)
        else:
            free = np.arange(2, max(2, I - 1))
            c = rng.choice(free, size=min(len(free), int(rng.integers(0, 20))), replace=False) if len(free) else np.zeros(0, dtype=np.int64)
            c = np.concatenate([[0], [1] if (u == 0 and I > 1) else [], c])
        cols.append(np.sort(c).astype(np.int64))
    col = np.concatenate(cols)
    val = rng.uniform(0.5, 5.0, size=len(col)).astype(np.float32)
    return col, val


def check_stats(dev, I, col, val):
    cnt, mean, glob, n_rated = dev_stats(dev, I, col, val)
    r_cnt, r_mean, r_gm, r_gs, r_nr = R.item_stats(I, col, val)
    mx = float(np.abs(val).max()) if len(val) else 0.0
    assert np.array_equal(cnt, r_cnt) and n_rated == r_nr
    assert np.all(np.abs(mean - r_mean) <= R.stat_bound(r_cnt, mx)), np.abs(mean - r_mean).max()
    assert (mean[r_cnt == 0] == 0).all()
    assert abs(glob[0] - r_gm) <= R.stat_bound(len(val), mx) and abs(glob[1] - r_gs) <= R.stat_bound(len(val), mx), (glob, r_gm, r_gs)
    return cnt


# ---------------------------------------------------------------- rk_heur_item_stats
@pytest.mark.parametrize("U", USERS)
@pytest.mark.parametrize("I", ITEMS)
def test_item_stats(gpu_device, I, U):
    col, val = craft_ratings(U, I, seed=100 * I + U)
    cnt = check_stats(gpu_device, I, col, val)
    assert cnt[0] == U
    if I > 2:
        assert cnt[1] == 1 and cnt[I - 1] == 0                                  # a single rating; an item nobody rated


def test_item_stats_dense_grid_stride_and_no_ratings(gpu_device):
    col, val = craft_ratings(300, 1025, seed=5, dense=True)                      # 307500 ratings: more than 1024 blocks x 256 threads
    assert len(col) > 1024 * 256
    check_stats(gpu_device, 1025, col, val)
    cnt, mean, glob, n_rated = dev_stats(gpu_device, 65, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))   # every item unrated
    assert not cnt.any() and not mean.any() and glob.tolist() == [0.0, 0.0] and n_rated == 0


def test_item_stats_integer_ratings_are_exact(gpu_device):
    """1..5 ratings: every sum is an integer below 2^53, so every order of addition gives the same mean, to the bit."""
    rng = np.random.default_rng(3)
    col = rng.integers(0, 257, size=20000)
    val = rng.integers(1, 6, size=20000).astype(np.float32)
    cnt, mean, glob, _ = dev_stats(gpu_device, 257, col, val)
    r_cnt, r_mean, r_gm, _, _ = R.item_stats(257, col, val)
    assert np.array_equal(cnt, r_cnt) and np.array_equal(mean, r_mean) and glob[0] == r_gm


# ---------------------------------------------------------------- rk_heur_popular
def dev_popular(dev, counts, k):
    I = len(counts)
    cnt = _t(counts, np.int32, dev)
    ids = torch.full((max(k, 1),), -9, dtype=torch.int32, device=dev)
    cs = torch.full((max(k, 1),), -9, dtype=torch.int32, device=dev)
    n = C.c_int32(-9)
    rc = _lib.lib().rk_heur_popular(I, _lib.ptr(cnt), k, _lib.ptr(ids), _lib.ptr(cs), C.byref(n), _lib.stream_ptr(dev))
    return rc, ids.cpu().numpy(), cs.cpu().numpy(), n.value


@pytest.mark.parametrize("I", ITEMS)
def test_popular(gpu_device, I):
    rng = np.random.default_rng(I)
    counts = rng.integers(0, 6, size=I)                                          # many ties, many unrated items
    counts[rng.integers(0, I)] = 1 << 25                                         # a count no float32 selection could keep exact
    if I > 3:
        counts[I - 2] = (1 << 25) + 1
    for k in (1, 11, I, I + 5):                                                  # k above the rated items, and above n_items
        rc, ids, cs, n = dev_popular(gpu_device, counts, k)
        r_ids, r_cs = R.popular(counts, k)
        assert rc == 0 and n == len(r_ids) == min(k, int((counts > 0).sum()))
        assert np.array_equal(ids[:n], r_ids) and np.array_equal(cs[:n], r_cs)
        assert (ids[n:k] == -1).all() and (cs[n:k] == 0).all()
    rc, ids, cs, n = dev_popular(gpu_device, np.zeros(I, dtype=np.int64), 11)    # every item unrated
    assert rc == 0 and n == 0 and (ids == -1).all()


# ---------------------------------------------------------------- rk_heur_generate
class Gen:
    """One rk_heur_generate call on crafted statistics: item i is rated (count 1, mean 1 + (i % 7) / 2) unless i % 3 == 2."""

    def __init__(self, dev, I):
        self.dev, self.I = dev, I
        i = np.arange(I)
        self.count = np.where(i % 3 == 2, 0, 1).astype(np.int64)
        self.mean = np.where(self.count > 0, 1.0 + (i % 7) / 2.0, 0.0)
        self.gmean, self.gstd = 3.6, 1.1
        self.count_t, self.mean_t = _t(self.count, np.int32, dev), _t(self.mean, np.float64, dev)

    def call(self, n, F, targets, selected, mode, cols=None, vals=None, seed=11, stream=0, with_stats=True, rows=None):
        rows = n if rows is None else rows
        out = torch.full((max(rows, 1), self.I), 7.0, dtype=torch.float32, device=self.dev)
        c_t = None if cols is None else _t(cols, np.int32, self.dev)
        v_t = None if vals is None else _t(vals, np.float64, self.dev)
        tg = (C.c_int32 * max(len(targets), 1))(*targets)
        sl = (C.c_int32 * max(len(selected), 1))(*selected)
        rc = _lib.lib().rk_heur_generate(n, self.I, F, tg, len(targets), sl if selected else None, len(selected), mode, self.gmean, self.gstd,
                                         _lib.ptr(self.mean_t) if with_stats else None, _lib.ptr(self.count_t) if with_stats else None,
                                         _lib.ptr(c_t), _lib.ptr(v_t), seed, stream, _lib.ptr(out), _lib.stream_ptr(self.dev))
        torch.cuda.synchronize(self.dev)
        return rc, out.cpu().numpy()


# (n_items, attack_num, filler_num, targets, selected): odd row lengths (every row alignment), one and many blocks,
# filler_num 1 and filler_num = the whole pool, 1 / 2 / 3 / 9 targets, more targets than rows, a target that is also selected
SHAPES = [
    (63, 7, 5, [3, 11], []),
    (64, 50, 62, [0, 63], []),                        # the pool is 62 items: every one chosen
    (65, 1, 1, [64], [0, 5]),
    (257, 7, 36, [1, 2, 3, 4, 5, 6, 7, 8, 9], [10, 200]),   # rate 0: no row rates a target
    (1025, 50, 36, [0, 7, 1024], [7, 300, 301]),      # 7 is a target and selected; rows 48, 49 rate no target
    (300, 50, 256, [9], list(range(20, 31))),         # filler_num at its limit, 11 selected ids
    (9, 4096, 6, [0, 8], [1]),                        # filler_num = the pool again, many rows
]
MODES = (R.GLOBAL, R.ITEM, R.ONES)


def craft_draws(I, n, F, excl, seed):
    rng = np.random.default_rng(seed)
    pool = np.setdiff1d(np.arange(I), excl)
    cols = np.stack([rng.choice(pool, size=F, replace=False) for _ in range(n)])
    vals = rng.normal(3.0, 2.5, size=(n, F))                                     # well outside [1, 5] on both sides
    vals.reshape(-1)[: min(6, vals.size)] = [0.5, 1.5, 2.5, 3.5, 4.5, 5.5][: min(6, vals.size)]   # exact ties: half to even
    return cols, vals


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_generate_replay_is_exact(gpu_device, shape, mode):
    I, n, F, tg, sel = SHAPES[shape]
    g = Gen(gpu_device, I)
    cols, vals = craft_draws(I, n, F, tg + sel, seed=shape)
    rc, out = g.call(n, F, tg, sel, mode, cols=cols, vals=None if mode == R.ONES else vals)
    assert rc == 0
    ref = R.profiles(n, I, tg, sel, cols, None if mode == R.ONES else vals)
    assert np.array_equal(out, ref)
    if mode != R.ONES and vals.size >= 6:
        assert out[0, cols[0, :min(F, 6)]].tolist() == [1.0, 2.0, 2.0, 4.0, 4.0, 5.0][: min(F, 6)]


def structure(out, n, I, F, tg, sel):
    """The exact part of an own-draw run: targets by the reference's slices, selected ids 5 on every row, filler_num distinct
    fillers per row outside both with integer values in 1..5, zeros everywhere else.  Returns the filler mask."""
    fixed = R.profiles(n, I, tg, sel, np.zeros((n, 0), dtype=np.int64), np.zeros((n, 0)))
    excl = np.zeros(I, dtype=bool)
    excl[tg + sel] = True
    assert np.array_equal(out[:, excl], fixed[:, excl])
    fill = out[:, ~excl]
    assert ((fill != 0).sum(axis=1) == F).all()
    assert np.isin(fill, [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]).all()
    mask = np.zeros(out.shape, dtype=bool)
    mask[:, ~excl] = fill != 0
    return mask


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_generate_own_draws_structure_and_columns(gpu_device, shape, mode):
    I, n, F, tg, sel = SHAPES[shape]
    g = Gen(gpu_device, I)
    seed, stream = 2023 + shape, (1 << 62) | 5
    rc, out = g.call(n, F, tg, sel, mode, seed=seed, stream=stream)
    assert rc == 0
    mask = structure(out, n, I, F, tg, sel)
    cols = R.draw_cols(seed, stream, n, F, I, tg + sel)
    want = np.zeros(out.shape, dtype=bool)
    want[np.arange(n)[:, None], cols] = True
    assert np.array_equal(mask, want)                                            # the restated integer RNG, to the bit
    if mode == R.ONES:
        assert (out[mask] == 1).all()
    rc2, again = g.call(n, F, tg, sel, mode, seed=seed, stream=stream)
    rc3, other = g.call(n, F, tg, sel, mode, seed=seed, stream=stream + 1)
    assert rc2 == 0 and rc3 == 0 and np.array_equal(out, again)                  # same (seed, stream): bit-identical
    if F < I - len(set(tg + sel)) or mode != R.ONES:
        assert not np.array_equal(out, other)                                    # the next stream: other draws
    structure(other, n, I, F, tg, sel)


def test_generate_own_draws_in_distribution(gpu_device):
    """n_items 64, attack_num 4096, filler_num 12, one target: a pool of P = 63 items, at a fixed seed.

    Inclusion.  Floyd's draw gives every 12-subset of the pool the same probability, so a pool item is in a row with
    probability p = 12 / 63, and rows are independent (their keys differ): its count over the 4096 rows is Binomial(4096, p),
    mean 4096 p = 780.2, standard deviation sqrt(4096 p (1 - p)) = 25.1.  Asserted: within 6 standard deviations (two-sided
    tail 2e-9 per item, 63 items).

    Values.  The N = 4096 * 12 filler values are independent; one is v in 1..5 with the probability p_v the normal CDF gives
    the rounding bin (R.value_probs), so the count of v is Binomial(N, p_v) and is asserted within 6 sqrt(N p_v (1 - p_v)) of
    N p_v.  GLOBAL: all N values from N(3.6, 1.1).  ITEM: the values at rated items of mean m from N(m, m) -- the scale IS the
    mean -- and those at unrated items from N(3.6, 1.1), each group with its own N (the group's size, given the columns)."""
    I, n, F, tg = 64, 4096, 12, [17]
    g = Gen(gpu_device, I)
    P = I - 1
    for mode in (R.GLOBAL, R.ITEM):
        rc, out = g.call(n, F, tg, [], mode, seed=77, stream=1 << 62)
        assert rc == 0
        mask = structure(out, n, I, F, tg, [])
        p = F / P
        hits = mask.sum(axis=0)
        pool = np.setdiff1d(np.arange(I), tg)
        dev = np.abs(hits[pool] - n * p) / np.sqrt(n * p * (1 - p))
        print("inclusion: worst deviation", dev.max(), "standard deviations")
        assert dev.max() <= 6 and hits[tg[0]] == 0
        groups = {}                                                              # (mu, sd) -> the values drawn from it
        for i in pool:
            key = (g.mean[i], g.mean[i]) if (mode == R.ITEM and g.count[i] > 0) else (g.gmean, g.gstd)
            groups.setdefault(key, []).append(out[mask[:, i], i])
        assert len(groups) == (1 if mode == R.GLOBAL else 8)
        for (mu, sd), parts in groups.items():
            v = np.concatenate(parts)
            N, pv = len(v), R.value_probs(mu, sd)
            got = np.asarray([(v == k).sum() for k in range(1, 6)])
            sigma = np.sqrt(N * pv * (1 - pv))
            print("values", mode, mu, sd, N, got.tolist(), (N * pv).round(1).tolist())
            assert np.all(np.abs(got - N * pv) <= 6 * sigma + 1e-9), (mode, mu, sd, got, N * pv)


# ---------------------------------------------------------------- refusals: the code, and nothing written
def test_refusals_write_nothing(gpu_device):
    g = Gen(gpu_device, 65)
    ok = dict(n=7, F=5, targets=[3], selected=[4], mode=R.GLOBAL)
    cols, vals = craft_draws(65, 7, 5, [3, 4], seed=1)
    bad = [dict(targets=[65]), dict(targets=[-1]), dict(selected=[65]), dict(selected=[-2]), dict(F=0), dict(F=_lib.RK_HEUR_MAX_FILLER + 1),
           dict(F=64), dict(targets=[]), dict(targets=list(range(1, 60)) * 2), dict(selected=list(range(5, 64)) + list(range(5, 12))),
           dict(mode=3), dict(mode=-1), dict(n=0), dict(vals=vals), dict(cols=cols), dict(mode=R.ITEM, with_stats=False)]
    for kw in bad:
        a = dict(ok, **kw)
        rc, out = g.call(a["n"], a["F"], a["targets"], a["selected"], a["mode"], cols=a.get("cols"), vals=a.get("vals"),
                         with_stats=a.get("with_stats", True), rows=7)
        assert rc == EINVAL, kw
        assert (out == 7.0).all(), kw
        assert _lib.lib().rk_last_error()
    rc, out = Gen(gpu_device, 1).call(1, 1, [0], [], R.ONES)                     # n_items 1: the only item is the target, the pool is empty
    assert rc == EINVAL and (out == 7.0).all()
    rc, out = g.call(7, 63, [3], [4], R.ONES)                                    # the pool itself is accepted
    assert rc == 0 and (out != 7.0).all()
    assert dev_popular(gpu_device, np.ones(5, dtype=np.int64), 0)[0] == EINVAL
    rc, ids, cs, n = dev_popular(gpu_device, np.ones(5, dtype=np.int64), -3)
    assert rc == EINVAL and (ids == -9).all() and n == -9
    cnt = torch.full((4,), -7, dtype=torch.int32, device=gpu_device)
    rc = _lib.lib().rk_heur_item_stats(0, 0, None, None, _lib.ptr(cnt), None, None, None, _lib.stream_ptr(gpu_device))
    assert rc == EINVAL and (cnt.cpu().numpy() == -7).all()
