"""CPU tests of the KnnSelectUsers defender: the numpy restatement of its definition (tests/_knn_restate.py) against plain
float64, the variants the definition rules out, selection, the detection report, the registry / lazy-init contract, the
host-side refusals and the workflow hook."""
import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, defense, model, synth, workflow
from recad_amd.defense.knn_select_users import KnnSelectUsers, check_config
from recad_amd.defense.pca_select_users import flag_count
from recad_amd.evaluate import detection_quality
from recad_amd.utils import NotInstantiatedError
from tests import _knn_restate as R


def _csr(A):
    """(ptr, idx, val float32, n_items) of a dense integer matrix."""
    A = np.asarray(A)
    ptr = np.concatenate([[0], np.cumsum((A != 0).sum(axis=1))]).astype(np.int64)
    r, c = np.nonzero(A)
    return ptr, c.astype(np.int32), A[r, c].astype(np.float32), A.shape[1]


def _random(U, I, density, explicit, seed):
    rng = np.random.default_rng(seed)
    A = (rng.random((U, I)) < density).astype(np.int64)
    return A * rng.integers(1, 6, size=A.shape) if explicit else A


def _exact(A, k):
    """DegSim in float64: D / sqrt(n n^T), the mean of the k_eff largest off-diagonal entries of each row."""
    A = A.astype(np.float64)
    D, n = A @ A.T, (A * A).sum(axis=1)
    W = D / np.sqrt(np.maximum(np.outer(n, n), 1.0))
    U, k_eff = len(A), min(k, len(A) - 1)
    return np.array([np.sort(np.delete(W[u], u))[::-1][:k_eff].mean() for u in range(U)])


@pytest.mark.parametrize("explicit", [False, True])
def test_restatement_is_accurate(explicit):
    """w carries three roundings (r_u, r_v each one, the conversion is exact below 2^24, the two products one each: the
    issue counts three for w) and the mean one more: |degsim - exact| <= 5 * 2^-24 * exact."""
    for seed, (U, I, dens, k) in enumerate([(40, 60, 0.2, 5), (90, 50, 0.4, 25), (30, 200, 0.05, 128)]):
        A = _random(U, I, dens, explicit, seed)
        _, got = R.degsim(*_csr(A), k)
        want = _exact(A, k)
        assert np.all(np.abs(got.astype(np.float64) - want) <= 5 * 2.0 ** -24 * want), np.abs(got - want).max()


def test_mutations_are_rejected():
    A = np.array([[1, 1, 1, 0, 0, 0], [1, 1, 0, 1, 0, 0], [0, 1, 1, 1, 1, 0], [0, 0, 0, 0, 1, 1]])
    U, k = 4, 5                                    # k_eff = 3 < k
    topw, got = R.degsim(*_csr(A), k)
    assert np.all(topw[:, 3:] == 0) and np.all(topw[:, 0] > 0)
    D = A @ A.T
    r = R.rnorm(A)
    W = (D.astype(np.float32) * r[:, None]) * r[None, :]
    with_self = np.array([R.mean_of(-np.sort(-W[u]), 3) for u in range(U)])
    by_k = np.array([np.float32(float(got[u]) * 3 / k) for u in range(U)])
    assert np.all(with_self != got), "a user's own profile (w = 0.99999994 or 1) must not count as a neighbour"
    assert np.all(by_k != got), "the mean is over k_eff = min(k, U - 1) neighbours, not k"
    # summation order: 1 + 2^-24 is the midpoint of two fp32 neighbours; six terms of 2^-54 vanish one by one when they are
    # added last (descending) and reach 1.5 fp64 ulps when they are added first (ascending)
    top = np.array([1.0, 2.0 ** -24] + [2.0 ** -54] * 6, dtype=np.float32)
    assert R.mean_of(top, 8) == np.float32(0.125) and R.mean_of(top[::-1], 8) == np.float32(0.125) + np.float32(2.0 ** -26)


def test_large_dot_rounds_in_the_conversion():
    ptr = np.array([0, 1100, 2200, 2201])
    idx = np.r_[np.arange(1100), np.arange(1100), [5]].astype(np.int32)
    val = np.r_[np.full(2200, 127.0), [1.0]].astype(np.float32)
    A = R.dense(ptr, idx, val, 1100)
    D = A @ A.T
    assert D[0, 1] == 17741900 > 2 ** 24 and D[0, 0] < 2 ** 31
    assert R.first_violation(ptr, idx, val, 1100) is None
    topw, _ = R.degsim(ptr, idx, val, 1100, 2)
    assert topw[0].tolist() == [np.float32(0.99999994), np.float32(0.030151134)] and f"{topw[0, 1]:.8f}" == "0.03015113"
    assert topw[0, 0] == np.nextafter(np.float32(1), np.float32(0)), "identical profiles give 0.99999994, not 1"
    # 17 741 900 is even, so fp32 still holds it; with one 2 among the 127s the dot is odd and the conversion rounds
    D2 = R.dense(*R.large_dot_odd())
    D2 = D2 @ D2.T
    assert D2[0, 1] == 17726025 > 2 ** 24 and float(np.float32(D2[0, 1])) != D2[0, 1]


def test_restated_refusals():
    ptr, idx, I = np.array([0, 2, 4]), np.array([0, 3, 1, 2]), 4
    ok = np.array([1, 127, 5, 3], dtype=np.float32)
    assert R.first_violation(ptr, idx, ok, I) is None
    for bad in (0.0, 128.0, 2.5, -1.0, np.nan):
        v = ok.copy()
        v[2] = bad
        assert R.first_violation(ptr, idx, v, I) == (R.BAD_VALUE, 1)
    assert R.first_violation(ptr, np.array([0, 3, 2, 2]), ok, I) == (R.BAD_COLUMN, 1)
    assert R.first_violation(ptr, np.array([3, 0, 1, 2]), ok, I) == (R.BAD_COLUMN, 0)
    assert R.first_violation(ptr, np.array([0, 3, 1, 4]), ok, I) == (R.BAD_COLUMN, 1)
    n = 133153
    big = (np.array([0, n]), np.arange(n), np.full(n, 127, dtype=np.float32), n)
    assert n * 127 * 127 >= 2 ** 31 and R.first_violation(*big) == (R.BAD_NORM, 0)
    edge = 133144                                   # the longest row of 127s whose squared norm is below 2^31
    assert (edge + 1) * 127 * 127 >= 2 ** 31 > edge * 127 * 127
    assert R.first_violation(np.array([0, edge]), np.arange(edge), np.full(edge, 127, dtype=np.float32), n) is None


def test_selection():
    s = np.array([0.5, 0.25, 0.5, 0.0, -0.0, 0.25], dtype=np.float32)
    assert R.select(s, 4, "low") == [3, 4, 1, 5] and R.select(s, 3, "high") == [0, 2, 1]
    assert R.select(s, 0, "low") == [] and R.select(s, 6, "high") == [0, 2, 1, 5, 3, 4]
    with pytest.raises(ValueError):
        R.select(np.array([0.1, np.nan]), 1)
    over = next(U for U in range(51, 4000) if (50 / U) * U > 50)
    assert flag_count(50, over) == 51 and len(R.select(np.zeros(over), flag_count(50, over))) == 51


def test_detection_quality():
    q = detection_quality([10, 11, 3], 10, 14)
    assert q == {"precision": 2 / 3, "recall": 0.5, "f1": 2 * (2 / 3) * 0.5 / (2 / 3 + 0.5), "n_flagged": 3, "n_fake": 4,
                 "true_positives": 2}
    assert detection_quality([], 10, 14) == {"precision": 0.0, "recall": 0.0, "f1": 0.0, "n_flagged": 0, "n_fake": 4, "true_positives": 0}
    none_fake = detection_quality([1, 2], 10, 10)
    assert none_fake["recall"] == 0.0 and none_fake["precision"] == 0.0 and none_fake["f1"] == 0.0 and none_fake["n_fake"] == 0
    assert detection_quality([13, 12, 11, 10], 10, 14)["f1"] == 1.0
    # documented choice: an id outside [0, n_total) names nobody and is ignored; a repeated id counts once
    assert detection_quality([10, 10, 14, 99, -1], 10, 14) == detection_quality([10], 10, 14)
    assert detection_quality(np.array([10, 11]), 10, 14)["true_positives"] == 2
    with pytest.raises(ValueError):
        detection_quality([1], 15, 14)


def _tiny():
    d = synth.make("tiny")
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                               need_graph=False, device=torch.device("cpu"), seed=5)


def test_registry_defaults_and_lazy_init():
    assert model.factories["defender"]["KnnSelectUsers"] is KnnSelectUsers is defense.KnnSelectUsers
    cfg = default.MODEL["defender"]["KnnSelectUsers"]
    assert {k: cfg[k] for k in ("k", "attack_num", "select", "band", "schedule")} == {
        "k": 25, "attack_num": 50, "select": "low", "band": None, "schedule": "work"}
    lazy = model.from_config("defender", "KnnSelectUsers", attack_num=15, not_a_key=1)
    assert lazy.model_name == "KnnSelectUsers"
    assert lazy._init_config["attack_num"] == 15 and lazy._init_config["k"] == 25 and "not_a_key" not in lazy._init_config
    for call in (lambda: lazy.defense_step(), lambda: lazy.input_describe()):
        with pytest.raises(NotInstantiatedError):
            call()
    ds = _tiny()
    real = lazy.I(dataset=ds)
    assert real.I() is real and real.user_num == ds.n_users and real.item_num == ds.n_items
    pca = model.from_config("defender", "PCASelectUsers").I(dataset=ds)
    assert real.input_describe() == pca.input_describe() and real.output_describe() == pca.output_describe()
    assert real.reset(k=7)._init_config["k"] == 7
    assert real.scores is None and real.ranking is None
    with pytest.raises(_lib.HipCallError):
        real.defense_step()      # CPU device: no fallback


@pytest.mark.parametrize("key,value", [("select", "middle"), ("select", None), ("k", 0), ("k", 129), ("k", 2.5), ("band", 96),
                                       ("band", 32), ("band", 0), ("band", _lib.RK_KNN_MAX_BAND + 64), ("schedule", "random")])
def test_host_side_refusals_need_no_library(monkeypatch, key, value):
    def no_library(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    d = model.from_config("defender", "KnnSelectUsers", **{key: value}).I(dataset=_tiny())
    with pytest.raises(ValueError, match=key):
        d.defense_step()
    check_config(128, "high", _lib.RK_KNN_MAX_BAND, "natural")
    check_config(1, "low", 64, "work")


def test_defense_sets_detection_with_a_stub_defender():
    from tests.test_host_logic import _StubVictim

    class Stub:
        def I(self, **kw):
            return self

        def to(self, device):
            return self

        def input_describe(self):
            return {"defense_step": {"dataset": None}}

        def defense_step(self, dataset=None):
            return [dataset.n_users - 1, dataset.n_users - 2, 0]

    ds = _tiny()
    wf = workflow.from_config("defense", victim_data=ds, attack_data=None, victim=_StubVictim(),
                              attacker=workflow.RandomAttack(ds.n_items, attack_num=10, filler_num=5, seed=1),
                              defender=Stub(), rec_epoch=1, attack_epoch=0, device=torch.device("cpu"))
    res = wf.execute()
    assert set(res) == {"attacked", "defended", "n_flagged"} and res["n_flagged"] == 3
    assert wf.fake_dataset.n_users == ds.n_users + 10
    assert wf.detection == detection_quality([309, 308, 0], 300, 310) and wf.detection["true_positives"] == 2
    assert wf.detection["precision"] == 2 / 3 and wf.detection["recall"] == 0.2


def test_constructed_attack_is_flagged_entirely():
    """Four groups of ten genuine users who each rate 18 of their group's 20 items, and six fake profiles that rate the target
    (item 0, which group 0 owns) and five items nobody else has: a fake's best neighbours are the other fakes at 1/6, a
    genuine user's are its group at about 0.9.  The restatement alone must flag every fake, not a fraction."""
    rng = np.random.default_rng(11)
    A = np.zeros((46, 80 + 30), dtype=np.int64)
    for g in range(4):
        for u in range(10):
            A[g * 10 + u, g * 20 + rng.permutation(20)[:18]] = 1
    for f in range(6):
        A[40 + f, 0] = 1
        A[40 + f, 80 + 5 * f: 85 + 5 * f] = 1
    _, d = R.degsim(*_csr(A), 5)
    assert d[40:].max() < 0.2 < 0.7 < d[:40].min(), (d[40:].max(), d[:40].min())
    m = flag_count(6, 46)
    flagged = R.select(d, m, "low")
    assert set(range(40, 46)) <= set(flagged) and len(flagged) == m
    assert detection_quality(flagged, 40, 46)["recall"] == 1.0
    assert not set(range(40, 46)) & set(R.select(d, m, "high"))
