"""CPU tests of the UBA attacker's host side (recad_amd/attack/uba.py) and of the restatement the GPU tests compare against
(tests/_uba_restate.py): the registry, ``dsp`` against the reference's own DSP() runs (tests/golden/uba_dsp.npz), the elementwise
restatement against the reference's recorded positions (tests/golden/uba_prob_elementwise.npz), the identity between the literal
appended-rows ``@`` form and the weighted sum the kernels compute, and the refusals that fire before a device is asked for.

Tie-dependent cases.  In the elementwise mode the selected item's score is 125, the maximum, so it misses the top ten only when
ten or more other items were redrawn to 5, and then where np.argsort puts it among the equal scores is unspecified.  Those
cases (n_greater < 10 <= n_greater + n_equal) are excluded from the hit-or-miss comparison; their share may not exceed
MAX_TIE_SHARE = 10 %, which the generator asserted when it wrote the fixture (33 of 3000 there)."""
import numpy as np
import pytest

from recad_amd import _lib, default, model
from recad_amd.attack import uba as uba_mod
from recad_amd.utils import InstantiateFail

from . import _golden as G
from . import _uba_restate as R

MAX_TIE_SHARE = 0.10


def test_registry_and_defaults():
    assert model.factories["attacker"]["uba"] is uba_mod.UBA and issubclass(uba_mod.UBA, model.factories["attacker"]["aush"])
    d = default.MODEL["attacker"]["uba"]
    ref = {"attack_num": 50, "filler_num": 36, "lr_g": 0.01, "lr_d": 0.001, "optim_g": "adam", "optim_d": "adam", "selected_ids": [62],
           "ZR_ratio": 0.2, "budget": 6}                                          # recad/default.py:210-221
    assert {k: d[k] for k in ref} == ref
    t = d["target_user_ids"]
    assert len(t) == 50 == len(set(t)) and t[:5] == [741, 225, 289, 338, 308] and t[-3:] == [130, 836, 91] and sum(t) == 20828
    assert d["hops"] == "elementwise" and d["seed"] is None
    assert set(d) == set(ref) | {"target_user_ids", "hops", "seed", "logging_level", "device"}
    lazy = model.from_config("attacker", "uba", budget=3, path="work")
    assert lazy._pending["budget"] == 3 and lazy._pending["path"] == "work" and lazy.model_name == "uba"
    assert (_lib.RK_UBA_TRIALS, _lib.RK_UBA_TOPN) == (R.TRIALS, R.TOPN)


def test_limits_match_the_header():
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "recad_hip.h")).read()
    for name in ("RK_UBA_MAX_BUDGET", "RK_UBA_MAX_TARGETS", "RK_UBA_TRIALS", "RK_UBA_TOPN", "RK_UBA_LDS_USERS", "RK_UBA_ELEMENTWISE",
                 "RK_UBA_MATRIX", "RK_UBA_PATH_AUTO", "RK_UBA_PATH_LDS", "RK_UBA_PATH_WORK"):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == getattr(_lib, name), name


# ---------------------------------------------------------------- dsp against the reference's DSP()
def test_dsp_matches_every_recorded_run():
    g = G.load("uba_dsp")
    targets = g["target_user_ids"].tolist()
    n_ok = 0
    for k in range(len(g["prob"])):
        outcome, n = str(g["outcome"][k]), int(g["n_users_out"][k])
        if outcome == "ok" and n > 0:
            assert uba_mod.dsp(g["prob"][k], targets, int(g["attack_num"][k])) == g["users"][k, :n].tolist(), k
            n_ok += 1
        else:                                                # the reference raised, or returned nothing
            with pytest.raises(ValueError, match="all zero" if outcome == "AttributeError" else "no knapsack record|chose no user"):
                uba_mod.dsp(g["prob"][k], targets, int(g["attack_num"][k]))
    assert n_ok >= 6 and "AttributeError" in g["outcome"].tolist()
    assert sorted(set(g["n_users_out"].tolist()))[-1] == 100 and 5 in g["n_users_out"].tolist()     # the all-ones matrix: one user, five times


def test_dsp_reads_budget_columns_and_refuses_a_wrong_shape():
    p = np.zeros((3, 2))
    p[:, 1] = 1.0                                           # weight 1 each: the walk back from group 3 takes all three
    assert uba_mod.dsp(p, [7, 8, 9], 3) == [9, 8, 7]
    p8 = np.zeros((2, 8))
    p8[:, 7] = 0.5                                          # a column the reference's range(6) would never read
    assert uba_mod.dsp(p8, [4, 5], 2) == [5] * 7 + [4] * 7
    with pytest.raises(ValueError, match="one row per target user"):
        uba_mod.dsp(np.ones((2, 6)), [1, 2, 3], 3)


# ---------------------------------------------------------------- the restatement against the reference's positions
@pytest.fixture(scope="module")
def prob_golden():
    g = G.load("uba_prob_elementwise")
    mat = g["train_mat"].astype(np.float64)
    targets, s, budget = g["target_user_ids"].tolist(), int(g["selected_id"]), int(g["budget"])
    prob, n_tie, hits, ties = R.prob(mat, targets, s, budget, g["draws"], "elementwise")
    return g, mat, targets, s, budget, prob, n_tie, hits, ties


def test_elementwise_restatement_against_the_recorded_positions(prob_golden):
    g, mat, targets, s, budget, prob, n_tie, hits, ties = prob_golden
    assert hits.shape == g["positions"].shape == (budget, R.TRIALS, len(targets))
    share = n_tie / ties.size
    print("tie-dependent", n_tie, "of", ties.size)
    assert 0 < share <= MAX_TIE_SHARE
    assert np.array_equal((g["positions"] != 0)[~ties], hits[~ties])
    # prob_mat differs from the reference's only where a tie-dependent case fell the other way
    assert np.abs(prob - g["prob_mat"]).max() <= ties.sum(axis=1).max() / R.TRIALS
    quiet = ~ties.any(axis=1).T                              # (target, b) without a tie-dependent trial
    assert np.array_equal(prob[quiet], g["prob_mat"][quiet])
    # point 2 of the issue: the reference overwrote its first target user's row; the fixture keeps both matrices
    after = g["train_mat_after"]
    changed = np.nonzero((after != g["train_mat"]).any(axis=1))[0]
    assert changed.tolist() == [targets[0]] and after[targets[0], s] == 5


def test_redraw_restatement_layout(prob_golden):
    g, mat, targets, s, *_ = prob_golden
    ptr, col = R.side_layout(mat, targets, s)
    assert np.array_equal(ptr, uba_mod.side_layout(*_csr(mat)[:2], targets, s)) and ptr[-1] == g["draws"].shape[2]
    red, val = R.redraw(mat, targets, s, g["draws"][0, 0])
    others = np.setdiff1d(np.arange(mat.shape[0]), targets)
    assert np.array_equal(red[others], mat[others]) and (red[targets, s] == 5).all()
    assert np.array_equal((red[targets] != 0), (mat[targets] != 0) | (np.arange(mat.shape[1]) == s))
    assert val.min() >= 1 and val.max() <= 5


# ---------------------------------------------------------------- the weighted sum is the appended-rows product
def _seeded(U, I, n_targets, seed, share_items=False):
    rng = np.random.default_rng(seed)
    mat = np.zeros((U, I))
    for u in range(U):
        n = int(rng.integers(0, min(I, 24)))
        mat[u, rng.choice(I, size=n, replace=False)] = rng.integers(1, 6, size=n)
    targets = rng.choice(U, size=n_targets, replace=False).tolist()
    if share_items and n_targets > 1:
        mat[targets[1]] = mat[targets[0]]
    return mat, targets, rng


def _csr(mat):
    nz = mat != 0
    ptr = np.zeros(mat.shape[0] + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(nz.sum(axis=1))
    return ptr, np.nonzero(nz)[1].astype(np.int32), mat[nz].astype(np.float32)


@pytest.mark.parametrize("U,I,n_targets,b,seed", [(40, 33, 3, 1, 1), (96, 64, 12, 6, 2), (57, 65, 7, 3, 3)])
def test_weighted_sum_equals_the_literal_matrix_form(U, I, n_targets, b, seed):
    mat, targets, rng = _seeded(U, I, n_targets, seed, share_items=True)
    s = int(rng.integers(0, I))
    ptr, _ = R.side_layout(mat, targets, s)
    red, _ = R.redraw(mat, targets, s, rng.integers(1, 6, size=ptr[-1]))
    lit = R.scores_matrix_literal(red, targets, b)
    assert lit.shape == (n_targets, I) and lit.max() < 2.0 ** 53 and np.array_equal(lit, np.round(lit))
    assert np.array_equal(R.scores_matrix_weighted(red, targets, b), lit)
    # a deliberately wrong variant -- the copies counted, the original row forgotten -- is caught
    wrong = R.scores_matrix_weighted(red, targets, b, target_weight=b)
    assert not np.array_equal(wrong, lit)
    assert np.array_equal(R.scores_elementwise(red, targets), red[targets] ** 3)


def test_csc_is_the_transpose():
    mat, _, _ = _seeded(31, 17, 2, 9)
    ptr, idx, val = _csr(mat)
    colptr, crow, cval = uba_mod.rating_csc(31, 17, ptr, idx, val)
    back = np.zeros_like(mat)
    back[crow, np.repeat(np.arange(17), np.diff(colptr))] = cval
    assert np.array_equal(back, mat) and all(np.all(np.diff(crow[colptr[j]:colptr[j + 1]]) > 0) for j in range(17))


# ---------------------------------------------------------------- refusals before any device
class _Stub:
    def __init__(self, mat):
        self.mat = mat

    def info_describe(self):
        return {"n_users": self.mat.shape[0], "n_items": self.mat.shape[1], "train_mat": self.mat}


@pytest.mark.parametrize("kw,match", [
    (dict(target_user_ids=[]), "1..64 users"), (dict(target_user_ids=list(range(65))), "1..64 users"),
    (dict(target_user_ids=[1, 2, 1]), "twice"), (dict(target_user_ids=[96]), r"\[0, 96\)"), (dict(target_user_ids=[-1]), r"\[0, 96\)"),
    (dict(budget=0), "budget"), (dict(budget=_lib.RK_UBA_MAX_BUDGET + 1), "budget"), (dict(budget=2.5), "budget"),
    (dict(hops="cube"), "hops"), (dict(path="fast"), "path"), (dict(selected_ids=[64]), r"selected_ids\[0\]"),
    (dict(selected_ids=[]), r"selected_ids\[0\]"),
])
def test_refusals_fire_before_a_device_is_requested(monkeypatch, kw, match):
    def no_device():
        raise AssertionError("a device was requested before the settings were checked")

    monkeypatch.setattr(_lib, "require_gpu", no_device)
    mat = G.load("uba_prob_elementwise")["train_mat"].astype(np.float32)
    cfg = dict(target_user_ids=[3, 4], selected_ids=[62], seed=1)
    cfg.update(kw)
    with pytest.raises(InstantiateFail, match=match):
        model.from_config("attacker", "uba", **cfg).I(dataset=_Stub(mat))


def test_layout_refusals_without_a_device():
    with pytest.raises(ValueError, match="LDS path"):
        uba_mod.check_settings(_lib.RK_UBA_LDS_USERS + 1, 64, [3], [0], 6, "matrix", "lds")
    with pytest.raises(ValueError, match="2\\^53"):
        uba_mod.check_settings(1 << 24, 1 << 24, [3], [0], 6, "matrix")
    tu, budget, mode, path = uba_mod.check_settings(1 << 24, 1 << 24, [3], [5, 2], 6, "elementwise")
    assert tu.tolist() == [5, 2] and tu.dtype == np.int32 and (budget, mode, path) == (6, _lib.RK_UBA_ELEMENTWISE, _lib.RK_UBA_PATH_AUTO)
    with pytest.raises(InstantiateFail, match="dataset"):
        model.from_config("attacker", "uba").I()
