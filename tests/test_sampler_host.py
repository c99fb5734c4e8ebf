"""CPU tests of the samplers: the numpy restatement of recad_amd/csrc/sampler.hip (tests/_sampler_restate.py) against brute force
and against the uniform distribution it claims, and the host samplers of ImplicitData on a user who has interacted with every
item.  The GPU tests (test_input_pipeline_gpu.py) compare the kernels with this restatement element for element, so what is
established here about the restatement holds for the kernels.

Bounds.  Everything is an equality except the uniformity checks: every bin count of N = 200 000 draws over n bins lies within
5 sigma, sigma = sqrt(N p (1 - p)), p = 1 / n, of N p.  The seeds are fixed, so the outcome is deterministic; 5 sigma is a
condition set beforehand (about 6e-7 per bin under the hypothesis, some 2 200 bins in all), not a measured figure."""
import threading

import numpy as np
import pytest

from recad_amd import dataset, synth

from . import _sampler_restate as S

N_DRAWS = 200_000
SEEDS = (1, 2, 3, 2 ** 61 + 5)
SIZES = (2, 7, 61, 113)


def _crafted_rows(I):
    every = np.arange(I)
    rows = [[], [0], [I - 1], every[::2], every[1:], every[:-1], np.delete(every, I // 2)]
    for deg in sorted({1, 2, I // 3, I - 1} & set(range(1, I + 1))):
        rows += [every[:deg], every[I - deg:]]
    return [np.unique(np.asarray(r, dtype=np.int32)) for r in rows]


@pytest.mark.parametrize("I", [1, 2, 40, 257])
def test_rth_free_item_against_brute_force(I):
    for row in _crafted_rows(I):
        free = np.array(sorted(set(range(I)) - set(row.tolist())), dtype=np.int64)
        assert len(free) == I - len(row)
        # the row sits inside a longer index array, between two other rows, as in a CSR
        idx = np.concatenate([[0, I - 1], row, [0, I - 1]])
        r = np.arange(len(free))
        got = S.rth_free_item(idx, np.full(len(free), 2), np.full(len(free), 2 + len(row)), r)
        assert np.array_equal(got, free), (I, row.tolist())


def test_bounded_stays_below_n():
    for n in (1, 2, 3, 2 ** 31 - 1):
        r = np.array([0, 2 ** 32 - 1, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)
        got = S.bounded(r, n)
        assert (got >= 0).all() and (got < n).all(), (n, got)
        assert got[0] == 0 and got[3] == n - 1 and got[1] == 0   # the low 32 bits do not count; the top of the range is reached


def test_lower_bound_and_edge_user_against_numpy():
    rng = np.random.default_rng(3)
    a = np.sort(rng.integers(0, 50, 64))
    x = np.arange(-1, 52)
    assert np.array_equal(S.lower_bound(a, np.full(len(x), 5), np.full(len(x), 60), x), 5 + np.searchsorted(a[5:60], x, side="left"))
    ptr = np.array([0, 0, 0, 3, 3, 4, 9, 9, 9], dtype=np.int64)   # empty users at the start, in the middle and at the end
    assert np.array_equal(S.edge_user(8, ptr, np.arange(9)), [2, 2, 2, 4, 5, 5, 5, 5, 5])


def _within_5_sigma(counts, n_bins, what):
    n = int(counts.sum())
    p = 1.0 / n_bins
    dev = np.abs(counts - n * p) / np.sqrt(n * p * (1 - p))
    print(f"{what}: largest deviation {dev.max():.2f} sigma over {n_bins} bins, {n} draws")
    assert len(counts) == n_bins and dev.max() <= 5.0, (what, float(dev.max()))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", SIZES)
def test_bpr_users_are_uniform(n, seed):
    ptr, idx = S.csr_of([[u % 2] for u in range(n)])
    users, _, _, valid, _ = S.bpr_sample(n, 2, ptr, idx, N_DRAWS, seed)
    assert valid.all()
    _within_5_sigma(np.bincount(users, minlength=n), n, f"bpr users n={n} seed={seed}")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", SIZES)
def test_bpr_positives_are_uniform_within_a_row(n, seed):
    row = np.delete(np.arange(n + 1), n // 2)     # n positives out of n + 1 items
    ptr, idx = S.csr_of([row])
    _, pos, neg, valid, _ = S.bpr_sample(1, n + 1, ptr, idx, N_DRAWS, seed)
    assert valid.all() and (neg == n // 2).all()
    _within_5_sigma(np.bincount(np.searchsorted(row, pos), minlength=n), n, f"bpr positives n={n} seed={seed}")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", SIZES)
def test_pointwise_negatives_are_uniform_within_the_complement(n, seed):
    I = n + 8
    row = np.linspace(0, I - 1, 8).astype(np.int64)       # 8 positives spread over the catalogue, first and last item included
    free = np.setdiff1d(np.arange(I), row)
    ptr, idx = S.csr_of([row])
    ratio = N_DRAWS // 8
    users, items, labels = S.pointwise_sample(1, I, ptr, idx, ratio, seed)
    negs = items[labels == 0]
    assert len(negs) == N_DRAWS and np.isin(negs, free).all() and (users == 0).all()
    _within_5_sigma(np.bincount(np.searchsorted(free, negs), minlength=n), n, f"pointwise negatives n={n} seed={seed}")


def test_the_dense_case_reaches_the_fallback():
    """64 rejections fail on a row of 39 out of 40 items with probability (39/40)^64 = 19.8 %: between 10 % and 30 % of the draws
    on such rows must be flagged, both on a graph of nothing but such rows and on the 39-item rows of the mixed dense case."""
    every = np.arange(S.DENSE_I)
    ptr, idx = S.csr_of([np.delete(every, f) for f in (0, 17, 39, 1, 38, 20, 9, 31)])
    users, pos, neg, valid, fb = S.bpr_sample(8, S.DENSE_I, ptr, idx, 4096, 12345)
    print(f"all rows of 39: fallback on {fb.sum()} of 4096 draws")
    assert 0.10 * 4096 <= fb.sum() <= 0.30 * 4096
    assert valid.all() and np.array_equal(neg, np.array([0, 17, 39, 1, 38, 20, 9, 31])[users]) and (pos != neg).all()
    ptr, idx = S.dense_case()
    users, pos, neg, valid, fb = S.bpr_sample(8, S.DENSE_I, ptr, idx, 4096, 12345)
    on39 = users <= 2
    print(f"dense case: fallback on {fb.sum()} draws, {fb[on39].sum()} of the {on39.sum()} on the rows of 39")
    assert 0.10 * on39.sum() <= fb[on39].sum() <= 0.30 * on39.sum()
    assert not fb[np.isin(users, [4, 5, 6, 7])].any()
    # whichever way the negative was found, it is outside the row and the positive inside it
    keys = set((np.repeat(np.arange(8), np.diff(ptr)) * S.DENSE_I + idx).tolist())
    ok = valid == 1
    assert np.array_equal(ok, ~np.isin(users, [S.DENSE_ROWS["full"], S.DENSE_ROWS["empty"]]))
    assert all((u * S.DENSE_I + p) in keys and (u * S.DENSE_I + g) not in keys for u, p, g in zip(users[ok], pos[ok], neg[ok]))
    assert (pos[~ok] == 0).all() and (neg[~ok] == 0).all()


def test_restated_samplers_keep_the_semantics_on_the_sparse_graph():
    ptr, idx = S.sparse_case()
    U, I = len(ptr) - 1, 200
    keys = set((np.repeat(np.arange(U), np.diff(ptr)) * I + idx).tolist())
    users, pos, neg, valid, fb = S.bpr_sample(U, I, ptr, idx, 5000, 11)
    assert not fb.any() and np.array_equal(valid == 1, np.diff(ptr)[users] > 0)
    ok = valid == 1
    assert all((u * I + p) in keys and (u * I + g) not in keys for u, p, g in zip(users[ok], pos[ok], neg[ok]))
    users, items, labels = S.pointwise_sample(U, I, ptr, idx, 4, 11)
    assert len(users) == 5 * len(idx) and np.array_equal(users[::5], np.repeat(np.arange(U), np.diff(ptr)))
    assert np.array_equal(items[::5], idx) and (labels[::5] == 1).all() and labels.sum() == len(idx)
    assert all(((u * I + i) in keys) == (l == 1) for u, i, l in zip(users, items, labels))


# ---------------------------------------------------------------- a user who has interacted with every item
FULL_USER = S.FULL_USER


def _tiny_with_a_full_user(sample):
    return S.tiny_with_a_full_user(sample, "cpu", "numpy")


def test_pointwise_host_sampler_with_a_full_user():
    ds = _tiny_with_a_full_user("pointwise")
    tp, ti = ds.train_csr_sorted()
    assert tp[FULL_USER + 1] - tp[FULL_USER] == ds.n_items == 200
    users, items, labels = ds.pointwise_sample()
    assert items.min() >= 0 and items.max() < ds.n_items
    keys = set((np.repeat(np.arange(ds.n_users), np.diff(tp)) * ds.n_items + ti).tolist())
    assert all(((u * ds.n_items + i) in keys) == (l == 1) for u, i, l in zip(users, items, labels))
    mine = users == FULL_USER
    assert mine.sum() == ds.n_items and (labels[mine] == 1).all()           # its positives, and no negative row
    ratio, deg = ds.config["negative_ratio"], np.diff(tp)
    others = np.delete(np.arange(ds.n_users), FULL_USER)
    assert np.array_equal(np.bincount(users[labels == 0], minlength=ds.n_users)[others], deg[others] * ratio)
    assert labels.sum() == len(ti)
    ep = ds.generate_epoch()
    assert len(ep["users"]) == len(users) and int(ep["items"].max()) < ds.n_items


def test_pairwise_host_sampler_with_a_full_user_terminates():
    ds = _tiny_with_a_full_user("pairwise")
    out = []
    th = threading.Thread(target=lambda: out.append(ds.pairwise_sample()), daemon=True)
    th.start()
    th.join(60)            # returns in milliseconds; an endless rejection loop is reported instead of hanging the suite
    assert out, "pairwise_sample did not return: the rejection loop cannot end for a user without a free item"
    users, pos, neg = out[0]
    assert len(users) > 0.9 * ds.traindataSize and FULL_USER not in users
    keys = set(ds._net_keys.tolist())
    assert all((u * ds.n_items + p) in keys and (u * ds.n_items + g) not in keys for u, p, g in zip(users, pos, neg))
    assert neg.min() >= 0 and neg.max() < ds.n_items


def test_host_samplers_unchanged_without_a_full_user():
    """the filters drop nothing on a graph without such a user, so the random streams and the epochs stay what they were"""
    d = synth.make("tiny")
    mk = lambda s: dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], need_graph=False,
                                       device="cpu", sample=s, graph_source="train", sampler="numpy", seed=3)
    ds = mk("pointwise")
    deg = np.diff(ds.train_csr_sorted()[0])
    users, items, labels = ds.pointwise_sample()
    assert len(users) == 5 * deg.sum() and np.array_equal(np.bincount(users[labels == 0], minlength=ds.n_users), 4 * deg)
    ds = mk("pairwise")
    rng = np.random.default_rng(3)
    drawn = rng.integers(0, ds.n_users, ds.traindataSize)
    assert np.array_equal(ds.pairwise_sample()[0], drawn[np.diff(ds._net[0])[drawn] > 0])
