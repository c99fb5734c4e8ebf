"""CPU tests of the UserKNN victim: the numpy restatement of its definition (tests/_userknn_restate.py) against plain float64
within the stated bounds, the variants the definition rules out, the degeneracy of the normalised form on implicit data, the
neighbour weights against the DegSim definition, a constructed push attack the restated model must reward, the registry /
lazy-init contract, the host-side refusals and the refusal to run on the CPU."""
import functools

import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, model, synth, victim
from recad_amd.utils import NotInstantiatedError
from recad_amd.victim._fit_once import FitOnceVictim
from recad_amd.victim.userknn import UserKNN, check_config
from tests import _knn_restate as K
from tests import _userknn_restate as R

NAMES = ("rk_userknn_scores", "rk_userknn_pair_scores")


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


@functools.lru_cache(maxsize=None)
def _tiny_tables(kind, k):
    return R.neighbours(*_tiny_csr(kind), k)


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("k", [1, 5, 20, 128])
@pytest.mark.parametrize("kind", ["implicit", "ratings", "value127"])
def test_restatement_stays_within_the_bound(kind, k, normalize):
    """Un-normalised, ItemKNN's count: w carries at most five roundings, each term one more, the sum k - 1 more, one unit for the
    second order: |score - exact| <= (k + 6) * 2^-24 * sum_t w_t q_t.  Normalised: numerator k + 6, denominator k + 5 (five
    roundings of w, k - 1 adds, one unit), the quotient 1 and one unit for the cross terms: relative (2 k + 13) * 2^-24.  `exact`
    is the float64 evaluation of the same neighbour list."""
    csr = _tiny_csr(kind)
    nbr_id, nbr_w = _tiny_tables(kind, k)
    users = np.arange(300)
    got = R.scores(*csr, nbr_id, nbr_w, users, normalize).astype(np.float64)
    want = R.scores_exact(*csr, nbr_id, users, normalize)
    bound = ((2 * k + 13) if normalize else (k + 6)) * 2.0 ** -24 * want
    worst = np.max(np.abs(got - want) / np.maximum(bound, 1e-300))
    print(f"{kind} k={k} normalize={normalize}: worst |error| / bound = {worst:.3f}")
    assert np.all(np.abs(got - want) <= bound) and want.max() > 0
    assert np.array_equal(got == 0, want == 0), "an item no kept neighbour rated scores +0.0 in both"


# ------------------------------------------------------------------------------------------------------------ wrong variants
def _variant_tables(csr, k, higher_id=False, with_self=False, zero_overlap=False):
    """The neighbour tables under one of the orderings / candidate sets the definition rules out."""
    D, W = R.similarities(R.dense(*csr))
    U = D.shape[0]
    k_eff = min(k, U - (0 if with_self else 1))
    nbr_id, nbr_w = np.full((k, U), -1, dtype=np.int32), np.zeros((k, U), dtype=np.float32)
    for u in range(U):
        cand = np.arange(U) if zero_overlap else np.nonzero(D[u] > 0)[0]
        if not with_self:
            cand = cand[cand != u]
        cand = cand[np.lexsort((-cand if higher_id else cand, -W[u, cand].astype(np.float64)))][:k_eff]
        nbr_id[: len(cand), u], nbr_w[: len(cand), u] = cand, W[u, cand]
    return nbr_id, nbr_w


def _variant_scores(A, nbr_id, nbr_w, users, normalize=False, descending=False, fused=False, den_all_slots=False):
    """Scores of every item for `users` under one of the sums the definition rules out (all False: the definition itself)."""
    Af = A.astype(np.float32)
    n = len(users)
    s, den = np.zeros((n, A.shape[1]), dtype=np.float32), np.zeros((n, A.shape[1]), dtype=np.float32)
    slots = range(nbr_id.shape[0])
    for t in (reversed(slots) if descending else slots):
        v, w = nbr_id[t, users].astype(np.int64), nbr_w[t, users][:, None]
        ok = (v >= 0) & (v < A.shape[0])
        q = Af[np.where(ok, v, 0)]
        hit = ok[:, None] & (q != 0)
        wq = np.broadcast_to(w, q.shape)
        if fused:                                                      # the product of two fp32 is exact in float64: one rounding in all
            new = (s.astype(np.float64) + wq.astype(np.float64) * q.astype(np.float64)).astype(np.float32)
        else:
            new = (s + (wq * q).astype(np.float32)).astype(np.float32)
        s = np.where(hit, new, s)
        den = np.where(ok[:, None] if den_all_slots else hit, (den + wq).astype(np.float32), den)
    return R._finish(s, den, normalize)


def test_the_variant_walk_is_the_definition_when_nothing_is_varied():
    csr = _tiny_csr("ratings")
    nbr_id, nbr_w = _tiny_tables("ratings", 20)
    users = np.arange(300)
    for normalize in (False, True):
        a = _variant_scores(R.dense(*csr), nbr_id, nbr_w, users, normalize)
        assert np.array_equal(a.view(np.uint32), R.scores(*csr, nbr_id, nbr_w, users, normalize).view(np.uint32))


def test_ties_go_to_the_lower_id_on_tiny():
    csr = _tiny_csr("implicit")
    for k in (5, 20):
        _, w = _tiny_tables("implicit", k + 1)
        tied = int(np.sum((w[k] > 0) & (w[k] == w[k - 1])))
        ids, _ = _tiny_tables("implicit", k)
        other, _ = _variant_tables(csr, k, higher_id=True)
        differ = int(np.sum(np.any(ids != other, axis=0)))
        print(f"k={k}: {tied} of 300 users have a tie across the k-th place; ties to the higher id change {differ} users' lists")
        assert tied > 0 and differ >= tied
        D, W = R.similarities(R.dense(*csr))
        u = int(np.nonzero((w[k] > 0) & (w[k] == w[k - 1]))[0][0])
        kept, dropped = _tiny_tables("implicit", k + 1)[0][k - 1, u], _tiny_tables("implicit", k + 1)[0][k, u]
        assert W[u, kept] == W[u, dropped] and kept < dropped


def test_self_is_no_neighbour_on_tiny():
    csr = _tiny_csr("ratings")
    ids, w = _tiny_tables("ratings", 5)
    D, W = R.similarities(R.dense(*csr))
    assert np.all(np.abs(np.diag(W) - 1) <= 2.0 ** -22), "w_uu is 1 but for its roundings: every user's best match would be the user"
    assert not np.any(ids == np.arange(300)[None, :])
    other, other_w = _variant_tables(csr, 5, with_self=True)
    assert np.all(np.any(other == np.arange(300)[None, :], axis=0)) and np.all(w[0] < other_w[0])


def test_zero_overlap_candidates_are_not_kept():
    """Every user of tiny overlaps with at least 133 others, more than the largest k, so the full set cannot tell this variant
    apart; its first 60 users can: k_eff = 59 there, and nobody overlaps with all 59 others."""
    ptr, idx, val, I = _tiny_csr("implicit")
    full = R.dense(ptr, idx, val, I)
    assert int(((full @ full.T > 0).sum(axis=1) - 1).min()) > _lib.RK_KNN_MAX_K
    csr = (ptr[:61], idx[: ptr[60]], val[: ptr[60]], I)
    ids, w = R.neighbours(*csr, 128)
    D = R.dense(*csr) @ R.dense(*csr).T
    overlapping = (D > 0).sum(axis=1) - 1
    short = np.nonzero(overlapping < 59)[0]
    print(f"{len(short)} of the first 60 users of tiny overlap with fewer than 59 others (fewest: {overlapping.min()})")
    assert len(short) > 0, "the slice tells this variant apart"
    other, _ = _variant_tables(csr, 128, zero_overlap=True)
    for u in range(60):
        n = int(overlapping[u])
        assert np.all(ids[:n, u] >= 0) and np.all(ids[n:, u] == -1) and np.all(w[:n, u] > 0) and np.all(w[n:, u].view(np.uint32) == 0)
        assert np.all(other[:59, u] >= 0) and np.all(other[59:, u] == -1), "the variant fills every slot up to k_eff"
    # and on a matrix small enough to read: user 2 shares no item with anybody, user 3 only with user 0
    A = np.array([[2, 3, 3, 0, 0], [0, 1, 1, 0, 0], [0, 0, 0, 0, 4], [5, 0, 0, 1, 0]])
    small, _ = R.neighbours(*_csr(A), 3)
    assert small[:, 2].tolist() == [-1, -1, -1] and small[:, 3].tolist() == [0, -1, -1] and small[:, 0].tolist()[2] == -1


def test_scores_sum_in_ascending_slot_order_to_the_bit():
    """1 + 2^-24 is the midpoint of two fp32 neighbours (ties to even: 1), so adding 2^-24 terms one by one after a 1 leaves 1,
    while adding them first carries: the order of the sum is part of the definition."""
    A = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]])
    nbr_id = np.array([[1], [2], [3]], dtype=np.int32).repeat(4, axis=1)
    nbr_w = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], dtype=np.float32).repeat(4, axis=1)
    got = R.scores(*_csr(A), nbr_id, nbr_w, [0])[0, 0]
    down = _variant_scores(A, nbr_id, nbr_w, np.array([0]), descending=True)[0, 0]
    assert got == np.float32(1.0) and down == np.float32(1.0 + 2.0 ** -23) and got.view(np.uint32) != down.view(np.uint32)
    norm = R.scores(*_csr(A), nbr_id, nbr_w, [0], True)[0]
    assert norm[0] == np.float32(1.0) and np.all(norm[1:].view(np.uint32) == 0), "den = 0: +0.0"
    pairs = R.pair_scores(*_csr(A), nbr_id, nbr_w, [0, 0, 4, -1, 0], [0, 3, 0, 0, 4])
    assert pairs.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0], "an id out of range scores 0.0"
    # on tiny too: the descending walk changes bits of ordinary scores
    csr = _tiny_csr("ratings")
    ids, w = _tiny_tables("ratings", 20)
    users = np.arange(300)
    a, b = R.scores(*csr, ids, w, users), _variant_scores(R.dense(*csr), ids, w, users, descending=True)
    assert int(np.sum(a.view(np.uint32) != b.view(np.uint32))) > 0


def test_a_fused_multiply_add_changes_bits():
    csr = _tiny_csr("ratings")
    ids, w = _tiny_tables("ratings", 20)
    users = np.arange(300)
    a, b = R.scores(*csr, ids, w, users), _variant_scores(R.dense(*csr), ids, w, users, fused=True)
    differ = int(np.sum(a.view(np.uint32) != b.view(np.uint32)))
    print(f"a fused multiply-add changes {differ} of {a.size} scores of tiny (ratings, k = 20)")
    assert differ > 0
    # and by hand: s = 3, w = 1 + 2^-23, q = 5: w q = 5 + 1.25 * 2^-21 rounds to 5 + 2^-21, and 8 + 2^-21 is a tie that goes to
    # the even 8; fused, 8 + 1.25 * 2^-21 lies above that midpoint and rounds to 8 + 2^-20
    w1 = np.float32(1.0 + 2.0 ** -23)
    two = np.float32(np.float32(3.0) + np.float32(w1 * np.float32(5.0)))
    one = np.float32(3.0 + float(w1) * 5.0)
    assert two == np.float32(8.0) and one == np.float32(8.0 + 2.0 ** -20)


def test_the_denominator_runs_over_the_raters_of_the_item_only():
    csr = _tiny_csr("ratings")
    ids, w = _tiny_tables("ratings", 20)
    users = np.arange(300)
    a = R.scores(*csr, ids, w, users, True)
    b = _variant_scores(R.dense(*csr), ids, w, users, normalize=True, den_all_slots=True)
    assert int(np.sum(a.view(np.uint32) != b.view(np.uint32))) > 0
    slack = 1 + (2 * 20 + 13) * 2.0 ** -24
    assert a.max() <= 5.0 * slack and a[a > 0].min() >= 1.0 / slack, "a weighted average of ratings 1..5 lies in [1, 5]"
    assert b[b > 0].min() < 1.0, "over all k slots it is no average"


def test_normalised_scores_of_implicit_data_are_exactly_zero_or_one():
    """fl(w * 1) = w, so numerator and denominator are the same bits: the definition's known degeneracy."""
    csr = _tiny_csr("implicit")
    for k in (1, 20, 128):
        s = R.scores(*csr, *_tiny_tables("implicit", k), np.arange(300), True)
        bits = set(np.unique(s.view(np.uint32)).tolist())
        assert bits == {0, int(np.float32(1.0).view(np.uint32))}
        raw = R.scores(*csr, *_tiny_tables("implicit", k), np.arange(300), False)
        assert np.array_equal(s == 1.0, raw > 0), "exactly the reachable items"


@pytest.mark.parametrize("kind", ["implicit", "ratings", "value127"])
def test_neighbour_weights_are_the_topw_of_the_degsim_definition(kind):
    csr = _tiny_csr(kind)
    for k in (5, 50):
        topw, _ = K.degsim(*csr, k)
        _, w = _tiny_tables(kind, k)
        assert np.array_equal(topw.view(np.uint32), np.ascontiguousarray(w.T).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ the push
@functools.lru_cache(maxsize=None)
def _push(kind, k, normalize):
    """(HR@10 before, after, HR@20 before, after, eligible): 15 profiles, each the target plus the 30 most popular items,
    appended to `tiny`; with ratings the push rates the target 5 and the fillers 3."""
    ptr, idx, val, I = _tiny_csr(kind)
    target = 139
    assert int(np.sum(idx == target)) == 6
    popular = np.argsort(-np.bincount(idx, minlength=I), kind="stable")[:31]
    popular = popular[popular != target][:30]
    profile = np.sort(np.r_[popular, target]).astype(np.int32)
    stars = np.where(profile == target, 5.0, 3.0) if kind == "ratings" else np.ones(31)
    new_ptr = np.r_[ptr, ptr[-1] + 31 * np.arange(1, 16)]
    new_idx = np.r_[idx, np.tile(profile, 15)].astype(np.int32)
    new_val = np.r_[val, np.tile(stars, 15)].astype(np.float32)
    out = []
    for top in (10, 20):
        before, n = R.hit_ratio(ptr, idx, val, I, k, target, top, normalize=normalize)
        after, n_after = R.hit_ratio(new_ptr, new_idx, new_val, I, k, target, top, real_users=300, normalize=normalize)
        assert n == n_after == 294
        out += [before, after]
    return (*out, n)


@pytest.mark.parametrize("kind,k,normalize", [("implicit", 20, False), ("implicit", 50, False), ("ratings", 20, False),
                                              ("ratings", 50, False), ("ratings", 50, True)])
def test_constructed_push_raises_the_hit_ratio(kind, k, normalize):
    """The fake users become neighbours of the real ones who rated the popular items, and every one of them rated the target."""
    b10, a10, b20, a20, n = _push(kind, k, normalize)
    print(f"{kind} k={k} normalize={normalize}: HR@10 of item 139 over {n} eligible users {b10:.3f} -> {a10:.3f}, "
          f"HR@20 {b20:.3f} -> {a20:.3f}")
    assert n == 294 and a10 > b10 and a20 > b20


def test_constructed_push_on_normalised_implicit_data_is_degenerate():
    """Every reachable item scores 1.0, so the top-K is the K lowest unseen reachable ids: the push makes the target reachable
    but cannot lift it above the ties."""
    ptr, idx, val, I = _tiny_csr("implicit")
    b10, a10, b20, a20, n = _push("implicit", 20, True)
    print(f"implicit k=20 normalize=True: HR@10 {b10:.3f} -> {a10:.3f}, HR@20 {b20:.3f} -> {a20:.3f} over {n} users (degenerate)")
    s = R.scores(ptr, idx, val, I, *_tiny_tables("implicit", 20), np.arange(300), True)
    assert set(np.unique(s).tolist()) == {0.0, 1.0}
    assert n == 294 and a10 == b10 == 0.0 and a20 == b20 == 0.0, "item 139 has far more than 20 lower-numbered ties"


# ------------------------------------------------------------------------------------------------------------ plumbing
def _tiny():
    d = synth.make("tiny")
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                               need_graph=False, device=torch.device("cpu"), seed=5)


def test_registry_defaults_and_lazy_init():
    assert model.factories["victim"]["userknn"] is UserKNN is victim.UserKNN and "UserKNN" in victim.__all__
    assert issubclass(UserKNN, FitOnceVictim) and (UserKNN.label, UserKNN.state_noun) == ("UserKNN", "tables")
    cfg = default.MODEL["victim"]["userknn"]
    assert {k: cfg[k] for k in ("k", "normalize", "band")} == {"k": 50, "normalize": False, "band": None}
    lazy = model.from_config("victim", "userknn", k=7, not_a_key=1)
    assert lazy.model_name == "userknn" and lazy._init_config["k"] == 7 and "not_a_key" not in lazy._init_config
    for call in (lambda: lazy.train_step(), lambda: lazy.fit(), lambda: lazy.input_describe(), lambda: lazy.score_matrix(None, None),
                 lambda: lazy.forward(None, None)):
        with pytest.raises(NotInstantiatedError):
            call()
    ds = _tiny()
    real = lazy.I(dataset=ds)
    assert isinstance(real, FitOnceVictim)
    assert real.I() is real and (real.num_users, real.num_items) == (ds.n_users, ds.n_items) == (300, 200)
    assert not hasattr(real, "scoring_tables"), "EvalSession must keep refusing this victim"
    assert real.nbr_w.shape == (7, 300) and not real.nbr_w.requires_grad and real.nbr_w.dtype == torch.float32
    assert real.nbr_id.shape == (7, 300) and real.nbr_id.dtype == torch.int32 and bool((real.nbr_id == -1).all())
    assert real.fitted.tolist() == [0]
    assert [n for n, _ in real.named_parameters()] == ["nbr_w"] and set(real.state_dict()) == {"nbr_w", "nbr_id", "fitted"}
    assert next(real.parameters()).device.type == "cpu"
    fwd = real.input_describe()["forward"]
    assert len(fwd) == 2 and "users" in fwd and "items" in fwd
    assert real.output_describe()["train_step"] == {"loss": (float, [])}
    again = real.reset(k=9, normalize=True)
    assert again._init_config["k"] == 9 and again._init_config["normalize"] is True and not again._is_instantiate
    for call in (real.train_step, real.fit, lambda: real.forward(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)),
                 lambda: real.score_matrix(torch.zeros(1, dtype=torch.int32), torch.zeros(200))):
        with pytest.raises(_lib.HipCallError, match="no CPU fallback"):
            call()        # tables on the CPU: no fallback


@pytest.mark.parametrize("key,value", [("k", 0), ("k", 129), ("k", 2.5), ("k", -1), ("k", True), ("normalize", 1), ("normalize", 0),
                                       ("normalize", None), ("normalize", "yes"), ("band", 96), ("band", 32), ("band", 0),
                                       ("band", True), ("band", _lib.RK_USERKNN_MAX_BAND + 64)])
def test_host_side_refusals_need_no_library(monkeypatch, key, value):
    def no_library(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    m = model.from_config("victim", "userknn", **{key: value}).I(dataset=_tiny())
    assert m.nbr_w.shape == (0, 300)
    for call in (m.train_step, m.fit, lambda: m.forward(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)),
                 lambda: m.score_matrix(torch.zeros(1, dtype=torch.int32), torch.zeros(200))):
        with pytest.raises(ValueError, match=f"{key} = "):
            call()
    check_config(128, True, _lib.RK_USERKNN_MAX_BAND)
    check_config(1, False, 64)
    check_config(50, False, None)


def test_abi_and_header():
    assert _lib.ABI_VERSION == 11 and set(NAMES) <= set(_lib.EXPORTS), "an entry was added, nothing changed"
    assert len(_lib._SIGNATURES["rk_userknn_scores"]) == 14 and len(_lib._SIGNATURES["rk_userknn_pair_scores"]) == 14
    # 8 bytes a column (numerator and denominator) within 160 KiB less the 64 bytes left free
    assert _lib.RK_USERKNN_MAX_BAND % 64 == 0 and 8 * _lib.RK_USERKNN_MAX_BAND <= 160 * 1024 - 64
    assert _lib.RK_USERKNN_MAX_BAND == _lib.RK_RP3_MAX_BAND
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "recad_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in header
    assert f"#define RK_USERKNN_MAX_BAND {_lib.RK_USERKNN_MAX_BAND}\n" in header
    assert "#define RK_ABI_VERSION 11\n" in header
    assert header.count("transposed roles") >= 2, "the header says at both places that the fit is rk_itemknn_neighbors"
