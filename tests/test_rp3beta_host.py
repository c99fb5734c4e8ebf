"""CPU tests of the RP3beta victim: the numpy restatement of its definition (tests/_rp3_restate.py) against the float64 textbook
RP3beta within the counted bound, its scores inside the counted budget, the variants the definition rules out, a constructed push
attack that shows the popularity penalty, the registry / lazy-init contract, the host-side refusals and the refusal to run on the
CPU."""
import functools
import math

import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, model, synth, victim
from recad_amd.utils import NotInstantiatedError
from recad_amd.victim.rp3beta import RP3beta, check_config
from tests import _rp3_restate as R

EXPONENTS = [(1, 0), (1, 0.6), (0.8, 0.4), (2, 0.3)]
NAMES = ("rk_rp3_steps", "rk_rp3_factors", "rk_rp3_neighbors", "rk_rp3_scores", "rk_rp3_pair_scores")


def _csr(A):
    """(ptr, idx, val float32, n_items) of a dense integer matrix."""
    A = np.asarray(A)
    ptr = np.concatenate([[0], np.cumsum((A != 0).sum(axis=1))]).astype(np.int64)
    r, c = np.nonzero(A)
    return ptr, c.astype(np.int32), A[r, c].astype(np.float32), A.shape[1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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
@pytest.mark.parametrize("alpha,beta", EXPONENTS)
@pytest.mark.parametrize("kind", ["implicit", "ratings", "value127"])
def test_restatement_against_the_textbook_and_inside_the_budget(kind, alpha, beta):
    """Weights: S carries the quantisation of P (each entry off by at most 1/2, relative 2^-41 / p_min), the float64 products and
    the textbook's own float64 sums a few 2^-53 each, and then ONE fp32 rounding: |w - textbook| <= (2^-24 (1 + d) + d) textbook,
    d = 2^-41 / p_min + (U + 16) 2^-53.  Scores: (m + c) 2^-24 sum of terms against float64 on the same tables."""
    ptr, idx, val, I = _tiny_csr(kind)
    P, r, fa, fb = R.fit_parts(ptr, idx, val, I, alpha, beta)
    S = R.dots(ptr, idx, P, I)
    W, T = R.weights(S, fa, fb).astype(np.float64), R.textbook(ptr, idx, val, I, alpha, beta)
    off = (S > 0) & ~np.eye(I, dtype=bool)
    assert np.array_equal(S > 0, T > 0)
    p_min = float(np.min(R._power(np.asarray(val, dtype=np.float64) / np.repeat(r, np.diff(ptr)), alpha)))
    d = 2.0 ** -41 / p_min + (len(ptr) + 15) * 2.0 ** -53
    bound = 2.0 ** -24 * (1 + d) + d
    worst = float(np.max(np.abs(W[off] - T[off]) / T[off]))
    print(f"{kind} alpha={alpha} beta={beta}: worst relative weight difference {worst:.3e} (bound {bound:.3e}, p_min {p_min:.3e})")
    assert worst <= bound
    k = 20
    nbr_id, nbr_w = R.neighbours_from(S, R.weights(S, fa, fb), k)
    users = np.arange(0, 300, 3)
    A = R.dense(ptr, idx, val, I)
    got, m = R._walk(A, nbr_id, nbr_w, users)
    want = R.scores_exact(ptr, idx, val, I, nbr_id, users, alpha, beta)
    budget = R.score_budget(m, want)
    ratio = float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(budget, 1e-300)))
    print(f"  scores: worst |error| / budget = {ratio:.3f}, up to {int(m.max())} terms")
    assert np.all(np.abs(got - want) <= budget) and want.max() > 0 and 1 < m.max() <= 4094


def test_tables_are_padded_and_ordered():
    rng = np.random.default_rng(2)
    A = (rng.random((30, 12)) < 0.3) * rng.integers(1, 6, size=(30, 12))
    A[:, 7] = 0                                                        # an item nobody rated
    csr = _csr(A)
    nbr_id, nbr_w = R.neighbours(*csr, 20, 1, 0.6)
    assert nbr_id.shape == (20, 12) and nbr_id.dtype == np.int32 and nbr_w.dtype == np.float32
    assert np.all(nbr_id[11:] == -1) and np.all(_bits(nbr_w[11:]) == 0), "k_eff = I - 1 = 11"
    assert np.all(nbr_id[:, 7] == -1) and not np.any(nbr_id == 7)
    B = (A > 0).astype(np.int64)
    C = B.T @ B
    for i in range(12):
        n = int(np.sum(nbr_id[:, i] >= 0))
        assert n == int(np.sum(C[i] > 0)) - int(C[i, i] > 0)
        assert np.all(np.diff(nbr_w[:n, i]) <= 0) and np.all(nbr_w[:n, i] > 0) and i not in nbr_id[:, i]
        assert len(set(nbr_id[:n, i].tolist())) == n, "the ids of one list are distinct"
    one = R.neighbours(*_csr(np.array([[3], [1]])), 4, 1, 0.6)
    assert np.all(one[0] == -1) and one[0].shape == (4, 1), "I = 1: no candidates at all"
    P, r = R.steps(*csr[:3], 1)
    assert r.tolist() == A.sum(axis=1).tolist() and P.dtype == np.int64 and np.all(P >= 1) and np.all(P <= 2 ** 40)


def test_exponents_one_and_zero_do_not_call_pow():
    """alpha = 1: P = rint(2^40 q / r) from the IEEE quotient, integer-checkable; alpha = 0: every P is 2^40; factors alike."""
    ptr, idx, val, I = _tiny_csr("ratings")
    P1, r = R.steps(ptr, idx, val, 1)
    q, rr = val.astype(np.int64), np.repeat(r, np.diff(ptr))
    assert np.all(np.abs(P1 * rr - (q << 40)) <= rr // 2 + 1), "P r = 2^40 q up to the rounding of one division"
    assert np.all(R.steps(ptr, idx, val, 0)[0] == 2 ** 40)
    n = np.array([0, 1, 3, 7])
    fa, fb = R.factors(n, 1, 0)
    assert fa.tolist() == [0.0, 1.0, 1.0 / 3, 1.0 / 7] and fb.tolist() == [0.0, 1.0, 1.0, 1.0]


# ------------------------------------------------------------------------------------------------------- variants ruled out
def _weights(csr, alpha, beta, first=None):
    P, _, fa, fb = R.fit_parts(*csr, alpha, beta)
    S = R.dots(*csr[:2], P, csr[3], first=first)
    return S, R.weights(S, fa, fb), fa, fb


def test_wrong_variants_are_rejected():
    # items 1 and 2 are rated by the same users with the same values: w_01 == w_02 exactly, and k = 1 keeps one of them
    A = np.array([[2, 3, 3, 0, 0],
                  [1, 1, 1, 0, 0],
                  [0, 0, 0, 4, 0],
                  [5, 0, 0, 1, 0]])
    csr = _csr(A)
    S, W, fa, fb = _weights(csr, 1, 0.6)
    nbr_id, nbr_w = R.neighbours(*csr, 1, 1, 0.6)
    assert W[0, 1] == W[0, 2] > W[0, 3] > 0
    assert nbr_id[0, 0] == 1, "a tie goes to the LOWER id (the higher-id variant gives 2)"
    # a kept diagonal: item 3's only other candidate is item 0, and its own weight is larger
    assert S[3, 3] > 0 and W[3, 3] > W[3, 0] > 0 and nbr_id[0, 3] == 0
    assert np.all(nbr_id[0, :4] != np.arange(4))
    # zero-overlap candidates admitted: item 4 has no rater and item 3 overlaps only item 0, yet k_eff = 4
    full_id, full_w = R.neighbours(*csr, 4, 1, 0.6)
    assert full_id[:, 4].tolist() == [-1] * 4 and full_id[:, 3].tolist() == [0, -1, -1, -1]
    assert full_id[:, 0].tolist() == [1, 2, 3, -1], "an admitted zero-overlap candidate would fill the last slot with item 4"
    assert np.all(_bits(full_w[full_id < 0]) == 0)
    # beta applied to the ROW item: n_0 = 3 raters, n_3 = 2, so n_j^-beta and n_i^-beta differ
    scale = 2.0 ** -40
    assert full_w[2, 0] == np.float32(((float(S[0, 3]) * fa[0]) * fb[3]) * scale) != np.float32(((float(S[0, 3]) * fa[0]) * fb[0]) * scale)
    # the first step weighted by q: user 3 rates item 0 at 5, which would count its row five times in S_0j
    Sq = R.dots(*csr[:2], R.steps(*csr[:3], 1)[0], 5, first=csr[2])
    assert Sq[0, 3] == 5 * S[0, 3] and S[0, 3] == R.steps(*csr[:3], 1)[0][-1], "binarised: S_03 is user 3's P_33 once"
    # seen items are scored like any other; an item with no rated neighbour scores +0.0
    s = R.scores(*csr, full_id, full_w, [0, 2])
    assert s[0, 0] > 0 and s[0, 1] > 0 and _bits(s[0, 4]) == 0
    assert s[1, 0] == np.float32(full_w[0, 3] * np.float32(4)), "user 2 rated item 3 only: item 0 is in item 3's list"
    assert _bits(s[1, 3]) == 0 and _bits(s[1, 1]) == 0


def test_a_step_that_rounds_to_zero_is_kept_at_one():
    """User 0: item 0 at 1 star and eleven others at 127, r = 1398; at alpha = 4, (1 / 1398)^4 = 2.6e-13 is below 2^-41, so
    rint(2^40 p) = 0 and P = max(1, 0) = 1.  Item 11 is rated by user 0 only: without the max, S_{11,0} = 0 and item 0 would
    not be a candidate of item 11 although a walk leads there."""
    A = np.zeros((2, 13), dtype=np.int64)
    A[0, 0], A[0, 1:12] = 1, 127
    A[1, 12] = 3
    csr = _csr(A)
    P, r = R.steps(*csr[:3], 4)
    assert r[0] == 1398 and (1 / 1398) ** 4 * 2.0 ** 40 < 0.5 and P[0] == 1 and np.all(P[1:] > 1)
    S = R.dots(*csr[:2], P, 13)
    assert S[11, 0] == 1
    nbr_id, nbr_w = R.neighbours(*csr, 12, 4, 0.3)
    assert 0 in nbr_id[:, 11] and nbr_id[10, 11] == 0 and nbr_w[10, 11] > 0 and nbr_id[11, 11] == -1


def test_scores_sum_in_ascending_item_order():
    """1 + 2^-24 is the midpoint of two fp32 neighbours (ties to even: 1), so adding 2^-24 terms one by one after a 1 leaves 1,
    while adding them first carries: summing the user's items in descending order gives other bits."""
    nbr_id = np.full((1, 4), -1, dtype=np.int32)
    nbr_id[0, 1:] = 0                                                  # item 0 is the one neighbour of items 1, 2 and 3
    nbr_w = np.array([[0.0, 1.0, 2.0 ** -24, 2.0 ** -24]], dtype=np.float32)
    csr = _csr(np.array([[0, 1, 1, 1]]))
    up = R.scores(*csr, nbr_id, nbr_w, [0])[0, 0]
    down = R.scores(*csr, nbr_id, nbr_w, [0], descending=True)[0, 0]
    assert up == np.float32(1.0) and down == np.float32(1.0 + 2.0 ** -23) and _bits(up) != _bits(down)
    pairs = R.pair_scores(*csr, nbr_id, nbr_w, [0, 0, 1, -1, 0], [0, 3, 0, 0, 4])
    assert pairs.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0], "an id out of range scores 0.0"


# ------------------------------------------------------------------------------------------------------------ the push
@functools.lru_cache(maxsize=None)
def _push(beta, k):
    """(HR@10 of item 139 before, after, eligible users): 15 profiles, each the target plus the 30 most popular items, appended
    to `tiny`."""
    ptr, idx, val, I = _tiny_csr("implicit")
    target = 139
    assert int(np.sum(idx == target)) == 6
    popular = np.argsort(-np.bincount(idx, minlength=I), kind="stable")[:31]
    popular = popular[popular != target][:30]
    profile = np.sort(np.r_[popular, target]).astype(np.int32)
    new_ptr = np.r_[ptr, ptr[-1] + 31 * np.arange(1, 16)]
    new_idx = np.r_[idx, np.tile(profile, 15)].astype(np.int32)
    new_val = np.ones(len(new_idx), dtype=np.float32)
    before, n = R.hit_ratio(ptr, idx, val, I, k, 1, beta, target, 10)
    after, n_after = R.hit_ratio(new_ptr, new_idx, new_val, I, k, 1, beta, target, 10, real_users=300)
    assert n == n_after == 294
    return before, after, n


def test_constructed_push_raises_the_hit_ratio_and_beta_is_what_it_leans_on():
    """The fake profiles tie the target to the popular items.  With beta = 0.6 the popular items' own weights are pushed down, so
    the target -- still rare -- climbs into the top 10; at beta = 0 (P3alpha) the popular items keep their lead and the lift is
    smaller."""
    b6, a6, n = _push(0.6, 20)
    b0, a0, _ = _push(0.0, 20)
    print(f"HR@10 of item 139 over {n} eligible users at alpha = 1, k = 20: beta = 0.6: {b6:.3f} -> {a6:.3f}; "
          f"beta = 0 (P3alpha): {b0:.3f} -> {a0:.3f}")
    assert a6 > b6
    assert a0 - b0 < a6 - b6


# ------------------------------------------------------------------------------------------------------------ plumbing
def _tiny():
    d = synth.make("tiny")
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                               need_graph=False, device=torch.device("cpu"), seed=5)


def test_registry_defaults_and_lazy_init():
    assert model.factories["victim"]["rp3beta"] is RP3beta is victim.RP3beta and "RP3beta" in victim.__all__
    cfg = default.MODEL["victim"]["rp3beta"]
    assert {k: cfg[k] for k in ("alpha", "beta", "k", "band")} == {"alpha": 1.0, "beta": 0.6, "k": 100, "band": None}
    lazy = model.from_config("victim", "rp3beta", k=7, not_a_key=1)
    assert lazy.model_name == "rp3beta" and lazy._init_config["k"] == 7 and "not_a_key" not in lazy._init_config
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
    again = real.reset(k=9, beta=0.0)
    assert again._init_config["k"] == 9 and again._init_config["beta"] == 0.0 and not again._is_instantiate
    for call in (real.train_step, real.fit, lambda: real.forward(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)),
                 lambda: real.score_matrix(torch.zeros(1, dtype=torch.int32), torch.zeros(200))):
        with pytest.raises(_lib.HipCallError, match="no CPU fallback"):
            call()        # tables on the CPU: no fallback


@pytest.mark.parametrize("key,value", [("alpha", -0.1), ("alpha", 4.5), ("alpha", math.nan), ("alpha", math.inf), ("alpha", "1"),
                                       ("alpha", True), ("beta", -1), ("beta", 4.0001), ("beta", math.nan), ("beta", None),
                                       ("k", 0), ("k", 129), ("k", 2.5), ("k", -1), ("band", 96), ("band", 32), ("band", 0),
                                       ("band", _lib.RK_RP3_MAX_BAND + 64)])
def test_host_side_refusals_need_no_library(monkeypatch, key, value):
    def no_library(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    m = model.from_config("victim", "rp3beta", **{key: value}).I(dataset=_tiny())
    assert m.nbr_w.shape == (0, 200)
    for call in (m.train_step, m.fit, lambda: m.forward(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)),
                 lambda: m.score_matrix(torch.zeros(1, dtype=torch.int32), torch.zeros(200))):
        with pytest.raises(ValueError, match=f"{key} = "):
            call()
    check_config(0, 4, 128, _lib.RK_RP3_MAX_BAND)
    check_config(4.0, 0.0, 1, 64, n_users=_lib.RK_RP3_MAX_USERS - 1)
    check_config(1, 0.6, 100, None)


def test_too_many_users_are_refused_on_the_host(monkeypatch):
    class Big:
        def info_describe(self):
            return {"n_users": _lib.RK_RP3_MAX_USERS, "n_items": 10}

    def no_library(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError, match=f"{2 ** 23} users"):
        model.from_config("victim", "rp3beta", k=1).I(dataset=Big()).train_step()


def test_abi_and_header():
    assert _lib.ABI_VERSION == 11 and set(NAMES) <= set(_lib.EXPORTS)
    assert _lib.RK_RP3_MAX_BAND % 64 == 0 and _lib.RK_RP3_MAX_USERS == 2 ** 23
    # 8 bytes an accumulator beside the list scratch of 4160 bytes, within 160 KiB less the 64 bytes left free
    assert 8 * _lib.RK_RP3_MAX_BAND + 4160 <= 160 * 1024 - 64 < 8 * (_lib.RK_RP3_MAX_BAND + 64) + 4160
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "recad_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in header
    for name in ("RK_RP3_MAX_BAND", "RK_RP3_MAX_USERS"):
        assert f"#define {name} {getattr(_lib, name)}\n" in header
    assert "#define RK_ABI_VERSION 11\n" in header
