"""CPU tests of the iALS victim: the numpy restatement (tests/_ials_restate.py) against the textbook normal equations and a dense
least-squares solve of the weighted problem, the conditions that keep the GPU tests honest checked on every case of the table in
float64, the budgets against planted defects, the objective, a constructed push attack under the float64 sweeps, and the registry,
lazy construction and host-side refusals of victim/ials.py."""
import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, model, synth, victim
from recad_amd.utils import NotInstantiatedError
from recad_amd.victim.ials import IALS, check_config
from tests import _ials_restate as R


def _by(**want):
    keys = ("d", "n", "alpha", "lam", "ratings", "state")
    return next(c for c in R.CASES if all(c[keys.index(k)] == v for k, v in want.items()))


# ------------------------------------------------------------------------------------------------------ the restatement
def test_case_table_covers_the_issue():
    assert {c[0] for c in R.CASES} == set(R.DIMS) == {1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 127, 128}
    assert {c[1] for c in R.CASES} == {1, 7, 70, 300, 255, 256, 257, 517} and (R.CHUNK, R.GRAM_ROWS) == (64, 256)
    assert {c[2:4] for c in R.CASES} >= {(0.0, 0.5), (1.0, 0.5), (40.0, 10.0)}
    assert [c[4] for c in R.CASES].count("127") == 1 and {c[4] for c in R.CASES} == {"ones", "1..5", "127"}
    assert {c[5] for c in R.CASES} == {"init", "swept"}
    for d in R.DIMS:                                # every dimension meets every pair, both rating kinds and both table states
        mine = [c for c in R.CASES if c[0] == d]
        assert {c[2:4] for c in mine} >= set(R.ALPHA_LAMBDA) and {c[4] for c in mine} >= set(R.RATINGS) and {c[5] for c in mine} == set(R.STATES)
    full = R.case(_by(d=16, n=300))
    assert np.diff(full["ptr"]).tolist() == [0, 1, 2, 3, 4, 5, 63, 64, 65, 197]
    assert np.diff(R.case(_by(d=16, n=7))["ptr"]).tolist() == [0, 1, 2, 3, 4, 5, 7]
    assert R.case(_by(ratings="127"))["val"].max() == 127 and R.case(_by(d=17, ratings="1..5"))["val"].max() == 5


def test_system_is_the_weighted_least_squares_problem():
    """x_u minimises sum_i c_ui (p_ui - x . y_i)^2 + lambda |x|^2 over ALL items: the normal equations written out densely, and
    numpy.linalg.lstsq of the stacked problem."""
    for c in (_by(d=3, n=70), _by(d=16, n=70), _by(d=17, n=300), _by(ratings="127")):
        k = R.case(c)
        Y, lam = k["Y"].astype(np.float64), float(np.float32(k["lam"]))
        Q = R.dense(k["ptr"], k["idx"], k["val"], k["n"])
        for u, row in enumerate(k["rows"]):
            cu = np.where(Q[u] > 0, R.confidence(Q[u], k["alpha"])[1].astype(np.float64), 1.0)
            p = (Q[u] > 0).astype(np.float64)
            A = Y.T @ (cu[:, None] * Y) + lam * np.eye(k["d"])
            b = Y.T @ (cu * p)
            assert np.allclose(A, row["A"], rtol=1e-12, atol=1e-15) and np.allclose(b, row["b"], rtol=1e-12, atol=1e-15)
            M = np.vstack([np.sqrt(cu)[:, None] * Y, np.sqrt(lam) * np.eye(k["d"])])
            x = np.linalg.lstsq(M, np.r_[np.sqrt(cu) * p, np.zeros(k["d"])], rcond=None)[0]
            assert np.allclose(x, row["x"], rtol=1e-8, atol=1e-12 * max(1.0, np.max(np.abs(x)))), (c, u)
            if row["n_u"] == 0:
                assert not row["x"].any() and not row["b"].any()


@pytest.mark.parametrize("d", R.DIMS)
def test_every_case_is_well_conditioned_and_the_walk_is_inside_the_budgets(d):
    """What keeps the GPU tests honest: kappa_2(A_u) <= 2^12, the fp32 walk inside the hard bound and under a relative 2^-10, and
    the walk's own G, A and b inside the budgets the device is held to."""
    for c in (c for c in R.CASES if c[0] == d):
        k = R.case(c)
        assert np.all(np.abs(k["G32"].astype(np.float64) - k["G64"]) <= k["e_G"]), c
        for row in k["rows"]:
            top = float(np.max(np.abs(row["x"]), initial=0.0))
            assert row["kappa"] <= R.KAPPA_CAP, (c, row["n_u"], row["kappa"])
            assert row["walk_err"] <= row["e_hard"] and row["walk_err"] <= R.REL_CAP * top, (c, row["n_u"], row["walk_err"], top)
            assert np.all(np.abs(row["A_walk"].astype(np.float64) - row["A"]) <= row["e_A"]), (c, row["n_u"])
            assert np.all(np.abs(row["b_walk"].astype(np.float64) - row["b"]) <= row["e_b"]), (c, row["n_u"])
            assert row["e_x"] <= 4 * row["e_hard"] + 2.0 ** -23 * top


def test_walk_refuses_a_bad_pivot():
    assert R.cholesky_walk(np.array([[1.0, 2.0], [2.0, 1.0]]))[1] == 1
    assert R.cholesky_walk(np.array([[np.nan, 0.0], [0.0, 1.0]]))[1] == 0
    assert R.cholesky_walk(np.array([[np.inf, 0.0], [0.0, 1.0]]))[1] == 0
    assert R.solve_walk(np.array([[0.0]]), np.array([1.0])) is None
    assert R.solve_walk(np.array([[4.0]]), np.array([2.0])).tolist() == [0.5]
    assert np.array_equal(R.solve_walk(np.eye(3) * 2, np.zeros(3)).view(np.uint32), np.zeros(3, dtype=np.uint32)), "+0.0 everywhere"


# ------------------------------------------------------------------------------------------------------ planted defects
def _defect_case():
    c = _by(d=17, n=300, alpha=40.0)
    k = R.case(c)
    u = len(k["rows"]) - 1                           # the longest row
    s = slice(k["ptr"][u], k["ptr"][u + 1])
    return k, k["rows"][u], k["idx"][s], k["val"][s]


def test_budgets_are_broken_by_the_defects():
    k, row, cols, q = _defect_case()
    Y, alpha, lam = k["Y"], k["alpha"], k["lam"]
    outside = lambda A: bool(np.any(np.abs(np.asarray(A, dtype=np.float64) - row["A"]) > row["e_A"]))
    assert not outside(row["A_walk"])
    # a dropped entry
    assert outside(R.system_walk(k["G32"], Y, cols[:-1], q[:-1], alpha)[0])
    assert not np.array_equal(R.b_walk(Y, cols[:-1], q[:-1], alpha), row["b_walk"])
    # c in place of c - 1 in A: alpha * q + 1 as the weight
    w, c = R.confidence(q, alpha)
    t = np.zeros_like(k["G32"])
    for e, i in enumerate(cols):
        t = t + (c[e] * Y[i])[:, None] * Y[i][None, :]
    assert outside(k["G32"] + t)
    # lambda left out
    no_lam = R.gram_walk(Y, 0.0)
    assert np.any(np.abs(no_lam.astype(np.float64) - k["G64"]) > k["e_G"]) and outside(R.system_walk(no_lam, Y, cols, q, alpha)[0])
    # G built from the listed rows only
    listed = R.gram_walk(Y[cols], lam)
    assert np.any(np.abs(listed.astype(np.float64) - k["G64"]) > k["e_G"]) and outside(R.system_walk(listed, Y, cols, q, alpha)[0])
    # b with w in place of c
    s = np.zeros(k["d"], dtype=np.float32)
    for e, i in enumerate(cols):
        s = s + w[e] * Y[i]
    assert not np.array_equal(s, row["b_walk"]) and np.any(np.abs(s - row["b"]) > row["e_b"])
    # a transposed triangular solve
    x_bad = R.solve_walk(row["A_walk"], row["b_walk"], transposed_solve=True)
    assert np.max(np.abs(x_bad - row["x"])) > row["e_x"] and np.max(np.abs(x_bad - row["x"])) > R.REL_CAP * np.max(np.abs(row["x"]))
    x_ok = R.solve_walk(row["A_walk"], row["b_walk"])
    assert np.max(np.abs(x_ok - row["x"])) <= row["e_x"]


# ------------------------------------------------------------------------------------------------------------ objective
def test_objective_equals_the_dense_form_and_never_rises():
    for c in (_by(d=3, n=70), _by(d=15, n=70, alpha=40.0), _by(d=33, n=7)):
        k = R.case(c)
        ptr, idx, val, n, alpha, lam = k["ptr"], k["idx"], k["val"], k["n"], k["alpha"], k["lam"]
        rng = np.random.default_rng(2)
        Y = 0.01 * rng.standard_normal((n, k["d"]))
        X = 0.01 * rng.standard_normal((len(ptr) - 1, k["d"]))
        last = R.objective64(ptr, idx, val, n, X, Y, alpha, lam)
        tp = R.transpose(ptr, idx, val, n)
        for step in range(6):                        # six half-sweeps
            if step % 2 == 0:
                X = R.half_sweep64(ptr, idx, val, Y, alpha, lam)
            else:
                Y = R.half_sweep64(*tp, X, alpha, lam)
            J = R.objective64(ptr, idx, val, n, X, Y, alpha, lam)
            sparse, rows = R.objective_rows64(ptr, idx, val, X, Y, alpha, lam)
            assert abs(sparse - J) <= R.j_budget(ptr, idx, val, n, X, Y, alpha, lam), (c, step)
            assert J <= last * (1 + 1e-12), (c, step, J, last)
            last = J
        assert last > 0


# ------------------------------------------------------------------------------------------------------------- the push
def _tiny_csr():
    d = synth.make("tiny")
    ptr, idx = (np.asarray(a) for a in d["train"])
    return ptr.astype(np.int64), idx.astype(np.int64)


def push_profiles(idx, target=139, n_fake=15, n_pop=5, n_items=200):
    popular = np.argsort(-np.bincount(idx, minlength=n_items), kind="stable")[:n_pop + 1]
    popular = popular[popular != target][:n_pop]
    return np.sort(np.r_[popular, [target]]), n_fake


def test_constructed_push_raises_the_hit_ratio():
    """15 profiles, each the target plus the 5 most popular items, appended to `tiny` (300 x 200), d = 16, alpha = 40, lambda = 10,
    five float64 sweeps from a seeded 0.01 N(0, 1) item table.  HR@10 of item 139 over the 294 users who have not rated it:
    0.000 before the push, 0.105 after (31 users)."""
    ptr, idx = _tiny_csr()
    target = 139
    prof, n_fake = push_profiles(idx, target)
    Y0 = (0.01 * np.random.default_rng(5).standard_normal((200, 16))).astype(np.float32)
    X, Y = R.fit64(ptr, idx, np.ones(len(idx)), 200, Y0, 40.0, 10.0, 5)
    before, n = R.hit_ratio(R.scores64(X, Y), ptr, idx, target, 10)
    ptr2 = np.r_[ptr, ptr[-1] + len(prof) * np.arange(1, n_fake + 1)]
    idx2 = np.r_[idx, np.tile(prof, n_fake)]
    X2, Y2 = R.fit64(ptr2, idx2, np.ones(len(idx2)), 200, Y0, 40.0, 10.0, 5)
    after, n_after = R.hit_ratio(R.scores64(X2, Y2), ptr2, idx2, target, 10, real_users=300)
    print(f"HR@10 of item {target} over {n} eligible users: {before:.3f} before the push, {after:.3f} after")
    assert n == n_after == 294 and before == 0.0 and after > 0.08      # measured: 0.000 -> 0.105


# ------------------------------------------------------------------------------------------------------------ plumbing
def _tiny():
    d = synth.make("tiny")
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                               need_graph=False, device=torch.device("cpu"), seed=5)


def test_import_without_a_gpu_and_constants():
    import recad_amd

    assert IALS is recad_amd.victim.IALS
    assert {"rk_ials_gram", "rk_ials_gram64", "rk_ials_system", "rk_ials_half_sweep", "rk_ials_objective"} <= set(_lib.EXPORTS)
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "recad_hip.h")).read()
    for name in ("RK_IALS_MAX_DIM", "RK_IALS_CHUNK", "RK_IALS_GRAM_ROWS", "RK_IALS_NOT_SPD"):
        assert f"#define {name} {getattr(_lib, name)}" in header
    assert (_lib.RK_IALS_MAX_DIM, _lib.RK_IALS_NOT_SPD) == (128, 7) and (R.CHUNK, R.GRAM_ROWS) == (_lib.RK_IALS_CHUNK, _lib.RK_IALS_GRAM_ROWS)
    assert _lib.ABI_VERSION == 11 and "#define RK_ABI_VERSION 11" in header


def test_registry_defaults_and_lazy_init():
    assert model.factories["victim"]["ials"] is IALS is victim.IALS and "IALS" in victim.__all__
    want = {"factor_num": 64, "alpha": 40.0, "reg_lambda": 10.0, "init_std": 0.01, "seed": None}
    assert {k: default.MODEL["victim"]["ials"][k] for k in want} == want
    lazy = model.from_config("victim", "ials", factor_num=16, seed=3, not_a_key=1)
    assert lazy.model_name == "ials" and lazy._init_config["factor_num"] == 16 and "not_a_key" not in lazy._init_config
    for call in (lambda: lazy.train_step(), lambda: lazy.input_describe(), lambda: lazy.scoring_tables(), lambda: lazy.forward(None, None)):
        with pytest.raises(NotInstantiatedError):
            call()
    ds = _tiny()
    real = lazy.I(dataset=ds)
    assert real.I() is real and (real.num_users, real.num_items) == (ds.n_users, ds.n_items) == (300, 200)
    assert real.scoring_tables_static is True
    assert real.user_emb.shape == (300, 16) and real.item_emb.shape == (200, 16) and not real.user_emb.any()
    assert not real.user_emb.requires_grad and not real.item_emb.requires_grad and real.item_emb.dtype == torch.float32
    assert 0.008 < float(real.item_emb.std()) < 0.012 and abs(float(real.item_emb.mean())) < 0.002
    assert real.sweeps_done.tolist() == [0] and not real.user_bias.any() and not real.item_bias.any()
    assert [n for n, _ in real.named_parameters()] == ["user_emb", "item_emb"]
    assert set(real.state_dict()) == {"user_emb", "item_emb", "user_bias", "item_bias", "sweeps_done"}
    again = model.from_config("victim", "ials", factor_num=16, seed=3).I(dataset=ds)
    assert torch.equal(again.item_emb, real.item_emb), "one seed, one item table"
    other = model.from_config("victim", "ials", factor_num=16, seed=4).I(dataset=ds)
    assert not torch.equal(other.item_emb, real.item_emb)
    torch.manual_seed(11)
    a = model.from_config("victim", "ials", factor_num=16).I(dataset=ds)
    torch.manual_seed(11)
    b = model.from_config("victim", "ials", factor_num=16).I(dataset=ds)
    assert torch.equal(a.item_emb, b.item_emb) and a.seed == b.seed is not None, "seed None draws from the global RNG at .I()"
    fwd = real.input_describe()["forward"]
    assert len(fwd) == 2 and "users" in fwd and "items" in fwd and real.input_describe()["train_step"] == {}
    assert real.output_describe()["train_step"] == {"loss": (float, [])}
    reset = real.reset(reg_lambda=3.0)
    assert reset._init_config["reg_lambda"] == 3.0 and reset._init_config["seed"] == 3 and not reset._is_instantiate
    for call in (real.train_step, real.scoring_tables, real.scoring_tables_key,
                 lambda: real.forward(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long))):
        with pytest.raises(_lib.HipCallError, match="no CPU fallback"):
            call()        # tables on the CPU: no fallback


@pytest.mark.parametrize("key,value", [("factor_num", 0), ("factor_num", 129), ("factor_num", -1), ("factor_num", 16.0), ("factor_num", True),
                                       ("factor_num", None), ("alpha", -1.0), ("alpha", float("nan")), ("alpha", float("inf")),
                                       ("alpha", 1e39), ("alpha", "40"), ("alpha", None), ("alpha", True), ("reg_lambda", 0),
                                       ("reg_lambda", -1.0), ("reg_lambda", float("nan")), ("reg_lambda", float("inf")), ("reg_lambda", 1e-60),
                                       ("reg_lambda", 1e39), ("reg_lambda", "10"), ("reg_lambda", None), ("reg_lambda", True),
                                       ("init_std", -0.1), ("init_std", float("nan")), ("seed", -1), ("seed", 1.5), ("seed", 2 ** 63)])
def test_host_side_refusals_need_no_library(monkeypatch, key, value):
    def no_library(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    m = model.from_config("victim", "ials", **{key: value}).I(dataset=_tiny())
    assert m.item_emb.numel() == 0 and m.user_emb.numel() == 0
    for call in (m.train_step, m.scoring_tables, lambda: m.forward(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long))):
        with pytest.raises(ValueError, match=key):
            call()
    check_config(64, 40.0, 10.0)
    check_config(1, 0, 0.5, 0.0, 0)
    check_config(128, 1, 1, 0.01, 2 ** 63 - 1)


def test_empty_catalogue_is_refused(monkeypatch):
    class Empty:
        def __init__(self, U, I):
            self.U, self.I = U, I

        def info_describe(self):
            return {"n_users": self.U, "n_items": self.I}

    for U, I in ((10, 0), (0, 10)):
        m = model.from_config("victim", "ials").I(dataset=Empty(U, I))
        assert m.item_emb.numel() == 0
        with pytest.raises(ValueError, match="empty catalogue"):
            m.train_step()
