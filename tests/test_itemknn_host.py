"""CPU tests of the ItemKNN victim: the numpy restatement of its definition (tests/_itemknn_restate.py) against plain float64
within the stated bound, the variants the definition rules out, a constructed push attack the restated model must reward, the
registry / lazy-init contract, the host-side refusals and the refusal to run on the CPU."""
import functools

import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, model, synth, victim
from recad_amd.utils import NotInstantiatedError
from recad_amd.victim.itemknn import ItemKNN, check_config, rows_that_fit
from tests import _itemknn_restate as R


def _csr(A):
    """(ptr, idx, val float32, n_items) of a dense integer matrix."""
    A = np.asarray(A)
    ptr = np.concatenate([[0], np.cumsum((A != 0).sum(axis=1))]).astype(np.int64)
    r, c = np.nonzero(A)
    return ptr, c.astype(np.int32), A[r, c].astype(np.float32), A.shape[1]


@functools.lru_cache(maxsize=None)
def _tiny_csr(kind):
    d = synth.make("tiny")
    ptr, idx = (np.asarray(a) for a in d["train"])
    if kind == "implicit":
        val = np.ones(len(idx), dtype=np.float32)
    elif kind == "ratings":
        val = np.asarray(synth.with_ratings(d)["train"][2], dtype=np.float32)
    else:
        val = np.full(len(idx), 127.0, dtype=np.float32)
    return ptr, idx.astype(np.int32), val, 200


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("k", [5, 20])
@pytest.mark.parametrize("kind", ["implicit", "ratings", "value127"])
def test_restatement_stays_within_the_bound(kind, k):
    """w carries at most five roundings (r_i, r_j, the conversion, two products), each term one more, the sum k - 1 more:
    |score - exact| <= (k + 6) * 2^-24 * sum_t w_t q_t, exact the float64 evaluation of the same neighbour list."""
    csr = _tiny_csr(kind)
    nbr_id, nbr_w = R.neighbours(*csr, k)
    users = np.arange(300)
    got = R.scores(*csr, nbr_id, nbr_w, users).astype(np.float64)
    want = R.scores_exact(*csr, nbr_id, users)
    bound = (k + 6) * 2.0 ** -24 * want
    worst = np.max(np.abs(got - want) / np.maximum(bound, 1e-300))
    print(f"{kind} k={k}: worst |error| / bound = {worst:.3f}")
    assert np.all(np.abs(got - want) <= bound) and want.max() > 0


def test_tables_of_tiny_have_ties_across_the_kth_place():
    """The id half of the order is exercised by ordinary data: some items' k-th and (k+1)-th candidates have the same w."""
    csr = _tiny_csr("implicit")
    for k in (5, 20):
        _, w = R.neighbours(*csr, k + 1)
        tied = int(np.sum((w[k] > 0) & (w[k] == w[k - 1])))
        print(f"k={k}: {tied} of 200 items have a tie across the k-th place")
        assert tied > 0


def test_tables_are_padded_and_ordered():
    rng = np.random.default_rng(2)
    A = (rng.random((30, 12)) < 0.3) * rng.integers(1, 6, size=(30, 12))
    A[:, 7] = 0                                                        # an item nobody rated
    nbr_id, nbr_w = R.neighbours(*_csr(A), 20)
    assert nbr_id.shape == (20, 12) and nbr_id.dtype == np.int32 and nbr_w.dtype == np.float32
    assert np.all(nbr_id[11:] == -1) and np.all(nbr_w[11:].view(np.uint32) == 0), "k_eff = I - 1 = 11"
    assert np.all(nbr_id[:, 7] == -1) and not np.any(nbr_id == 7)
    D = A.T @ A
    for i in range(12):
        n = int(np.sum(nbr_id[:, i] >= 0))
        assert n == int(np.sum(D[i] > 0)) - int(D[i, i] > 0)
        assert np.all(np.diff(nbr_w[:n, i]) <= 0) and np.all(nbr_w[:n, i] > 0) and i not in nbr_id[:, i]
    one = R.neighbours(*_csr(np.array([[3], [1]])), 4)
    assert np.all(one[0] == -1) and one[0].shape == (4, 1), "I = 1: no candidates at all"


def test_wrong_variants_are_rejected():
    # items 1 and 2 are rated by the same users with the same values: w_01 == w_02 exactly, and k = 1 keeps one of them
    A = np.array([[2, 3, 3, 0, 0],
                  [1, 1, 1, 0, 0],
                  [0, 0, 0, 4, 0],
                  [5, 0, 0, 1, 0]])
    csr = _csr(A)
    nbr_id, nbr_w = R.neighbours(*csr, 1)
    _, W = R.similarities(A)
    assert W[0, 1] == W[0, 2] > W[0, 3] > 0
    assert nbr_id[0, 0] == 1, "a tie goes to the LOWER id (the higher-id variant gives 2)"
    # self included: every item's best match would be itself, at w = 1 or 0.99999994
    assert np.all(W[np.arange(4), np.arange(4)] >= np.float32(0.99999994)) and np.all(nbr_id[0, :4] != np.arange(4))
    assert nbr_w[0, 0] == W[0, 1] < W[0, 0]
    # zero-overlap candidates admitted: item 4 has no rater and item 3 overlaps only item 0, yet k_eff = 4
    full_id, full_w = R.neighbours(*csr, 4)
    assert full_id[:, 4].tolist() == [-1] * 4 and full_id[:, 3].tolist() == [0, -1, -1, -1]
    assert full_id[:, 0].tolist() == [1, 2, 3, -1], "an admitted zero-overlap candidate would fill the last slot with item 4"
    assert np.all(full_w[full_id < 0].view(np.uint32) == 0)
    # a sum-normalised score divides by sum_t w_t: user 2 (who rated item 3 only, 4 stars) would score item 0 at exactly 4
    s = R.scores(*csr, full_id, full_w, [2])[0]
    assert s[0] == np.float32(W[0, 3] * np.float32(4)) and s[0] != np.float32(4)
    normalised = s[0] / full_w[:, 0].sum()
    assert normalised != s[0]
    assert s[3] == 0 and s[4] == 0 and s[1] == 0, "items with no rated neighbour score +0.0"
    # seen items are scored like any other
    s0 = R.scores(*csr, full_id, full_w, [0])[0]
    assert s0[0] > 0 and s0[1] > 0


def test_scores_sum_in_slot_order():
    """1 + 2^-24 is the midpoint of two fp32 neighbours (ties to even: 1), so adding 2^-24 terms one by one after a 1 leaves
    1, while adding them first would carry: the order of the sum is part of the definition."""
    nbr_id = np.array([[1], [2], [3]], dtype=np.int32).repeat(4, axis=1)
    nbr_w = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], dtype=np.float32).repeat(4, axis=1)
    A = np.array([[0, 1, 1, 1]])
    got = R.scores(*_csr(A), nbr_id, nbr_w, [0])[0, 0]
    assert got == np.float32(1.0) and np.float32(np.float32(2.0 ** -24) + np.float32(2.0 ** -24)) + np.float32(1) > 1
    pairs = R.pair_scores(*_csr(A), nbr_id, nbr_w, [0, 0, 1, -1, 0], [0, 3, 0, 0, 4])
    assert pairs.tolist() == [1.0, 1.0, 0.0, 0.0, 0.0], "an id out of range scores 0.0"


def test_constructed_push_raises_the_hit_ratio():
    """15 profiles, each the target plus the 30 most popular items, appended to `tiny`: the target becomes a neighbour of the
    items most users have rated.  The restated model's HR@10 of the target over the users who have not rated it must rise."""
    ptr, idx, val, I = _tiny_csr("implicit")
    k, target = 20, 139
    assert int(np.sum(idx == target)) == 6
    popular = np.argsort(-np.bincount(idx, minlength=I), kind="stable")[:31]
    popular = popular[popular != target][:30]
    profile = np.sort(np.r_[popular, target]).astype(np.int32)
    new_ptr = np.r_[ptr, ptr[-1] + 31 * np.arange(1, 16)]
    new_idx = np.r_[idx, np.tile(profile, 15)].astype(np.int32)
    new_val = np.ones(len(new_idx), dtype=np.float32)
    before, n = R.hit_ratio(ptr, idx, val, I, k, target, 10)
    after, n_after = R.hit_ratio(new_ptr, new_idx, new_val, I, k, target, 10, real_users=300)
    print(f"HR@10 of item {target} over {n} eligible users: {before:.3f} before the push, {after:.3f} after")
    assert n == n_after == 294 and after > before


# ------------------------------------------------------------------------------------------------------------ plumbing
def _tiny():
    d = synth.make("tiny")
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                               need_graph=False, device=torch.device("cpu"), seed=5)


def test_registry_defaults_and_lazy_init():
    assert model.factories["victim"]["itemknn"] is ItemKNN is victim.ItemKNN and "ItemKNN" in victim.__all__
    cfg = default.MODEL["victim"]["itemknn"]
    assert {k: cfg[k] for k in ("k", "band", "user_block")} == {"k": 50, "band": None, "user_block": None}
    lazy = model.from_config("victim", "itemknn", k=7, not_a_key=1)
    assert lazy.model_name == "itemknn" and lazy._init_config["k"] == 7 and "not_a_key" not in lazy._init_config
    for call in (lambda: lazy.train_step(), lambda: lazy.fit(), lambda: lazy.input_describe(), lambda: lazy.score_matrix(None, None),
                 lambda: lazy.forward(None, None)):
        with pytest.raises(NotInstantiatedError):
            call()
    ds = _tiny()
    real = lazy.I(dataset=ds)
    assert real.I() is real and (real.num_users, real.num_items) == (ds.n_users, ds.n_items) == (300, 200)
    assert not hasattr(real, "scoring_tables"), "EvalSession must keep refusing this victim"
    assert real.nbr_w.shape == (7, 200) and not real.nbr_w.requires_grad and real.nbr_w.dtype == torch.float32
    assert real.nbr_id.dtype == torch.int32 and bool((real.nbr_id == -1).all()) and real.fitted.tolist() == [0]
    assert [n for n, _ in real.named_parameters()] == ["nbr_w"] and set(real.state_dict()) == {"nbr_w", "nbr_id", "fitted"}
    assert next(real.parameters()).device.type == "cpu"
    fwd = real.input_describe()["forward"]
    assert len(fwd) == 2 and "users" in fwd and "items" in fwd
    assert real.output_describe()["train_step"] == {"loss": (float, [])}
    again = real.reset(k=9)
    assert again._init_config["k"] == 9 and not again._is_instantiate
    for call in (real.train_step, real.fit, lambda: real.forward(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)),
                 lambda: real.score_matrix(torch.zeros(1, dtype=torch.int32), torch.zeros(200))):
        with pytest.raises(_lib.HipCallError, match="no CPU fallback"):
            call()        # tables on the CPU: no fallback


@pytest.mark.parametrize("key,value", [("k", 0), ("k", 129), ("k", 2.5), ("k", -1), ("band", 96), ("band", 32), ("band", 0),
                                       ("band", _lib.RK_ITEMKNN_MAX_BAND + 64), ("user_block", 0), ("user_block", 17),
                                       ("user_block", 1.5)])
def test_host_side_refusals_need_no_library(monkeypatch, key, value):
    def no_library(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    m = model.from_config("victim", "itemknn", **{key: value}).I(dataset=_tiny())
    for call in (m.train_step, m.fit, lambda: m.forward(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)),
                 lambda: m.score_matrix(torch.zeros(1, dtype=torch.int32), torch.zeros(200))):
        with pytest.raises(ValueError, match=key):
            call()
    check_config(128, _lib.RK_ITEMKNN_MAX_BAND, 16)
    check_config(1, 64, 1)
    check_config(50, None, None)


def test_catalogue_limits():
    assert rows_that_fit(1) == _lib.RK_ITEMKNN_MAX_ITEMS // 16 and rows_that_fit(200) == 787
    assert rows_that_fit(70000) == 2 and rows_that_fit(_lib.RK_ITEMKNN_MAX_ITEMS) == 1 and rows_that_fit(_lib.RK_ITEMKNN_MAX_ITEMS + 1) == 0
    assert _lib.RK_ITEMKNN_MAX_ITEMS % 16 == 0 and _lib.RK_ITEMKNN_MAX_BAND % 64 == 0
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "recad_hip.h")).read()
    for name in ("RK_ITEMKNN_MAX_BAND", "RK_ITEMKNN_MAX_ITEMS", "RK_ITEMKNN_MAX_USER_BLOCK"):
        assert f"#define {name} {getattr(_lib, name)}\n" in header

    class Big:
        def info_describe(self):
            return {"n_users": 10, "n_items": _lib.RK_ITEMKNN_MAX_ITEMS + 1}

    class Wide(Big):
        def info_describe(self):
            return {"n_users": 10, "n_items": 70000}

    with pytest.raises(ValueError, match="at most"):
        model.from_config("victim", "itemknn", k=1).I(dataset=Big()).train_step()
    with pytest.raises(ValueError, match="user_block = 3"):
        model.from_config("victim", "itemknn", k=1, user_block=3).I(dataset=Wide()).train_step()
