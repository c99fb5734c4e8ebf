"""CPU tests of the SLIM victim: the numpy walk of the definition (tests/_slim_restate.py) in float64 against the optimisation
problem it solves (a falling objective, the KKT conditions, the exact minimiser of tiny problems), in fp32 against its own running
error bound on every input the GPU tests use, the wrong variants the walk must tell apart, constructed cases, a constructed push
attack the restated model must reward, the registry / lazy-init contract, the host-side refusals and the refusal to run on the
CPU."""
import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, model, synth, victim
from recad_amd.utils import NotInstantiatedError
from recad_amd.victim.slim import SLIM, check_config
from tests import _slim_restate as R

F64 = np.float64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the float64 walk
@pytest.mark.parametrize("n,U,l1,beta", [(65, 70, 1.0, 5.0), (64, 300, 0.0, 0.5), (200, 70, 5.0, 500.0), (3, 5, 0.0, 0.5)])
def test_objective_never_rises_and_kkt_holds(n, U, l1, beta):
    """Coordinate descent minimises f_j exactly along each coordinate, so f_j falls (to rounding: 1e-12 of its size) from sweep to
    sweep in every column; once the walk has stopped moving (600 sweeps) w >= 0, gradient + l1 = 0 on the support and >= 0 off it,
    to 1e-9 of the largest Gram entry."""
    G = R.matrix(R.gram(R.ratings(U, n, 2000 * n + 10 * U)), beta)
    trail = []
    W, Rm, info, _ = R.walk(G, l1, 600, dtype=F64, on_sweep=lambda s, W, Rm: trail.append(R.objective(G, W, l1)))
    f = np.array(trail)
    scale = np.maximum(np.abs(f).max(axis=0), 1.0)
    assert np.all(np.diff(f, axis=0) <= 1e-12 * scale[None, :])
    assert f[-1].min() < 0 or n < 64, "some column found a weight worth having"
    on, off = R.kkt(G, W, l1)
    tol = 1e-9 * float(np.abs(G).max())
    assert np.all(W >= 0) and np.all(np.diag(W) == 0) and on.max() <= tol and off.max() <= tol, (on.max(), off.max(), tol)
    assert np.allclose(Rm, G.astype(F64) - G.astype(F64).T @ W, rtol=0, atol=1e-9 * float(np.abs(G).max())), "r is the residual"


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_small_problems_reach_the_exact_minimiser(n):
    for U, l1, beta in ((5, 0.0, 0.5), (70, 1.0, 5.0), (70, 0.0, 0.5), (300, 5.0, 500.0), (9, 0.5, 1.0)):
        G = R.matrix(R.gram(R.ratings(U, n, 31 * n + U)), beta)
        W = R.walk(G, l1, 5000, dtype=F64)[0]
        for j in range(n):
            want = R.exact_minimiser(G, l1, j)
            assert np.allclose(W[:, j], want, rtol=1e-9, atol=1e-12), (U, l1, beta, j, W[:, j], want)


# ------------------------------------------------------------------------------------------------------------ the fp32 walk
@pytest.mark.parametrize("n", R.ITEMS)
def test_fp32_walk_holds_its_error_bound_on_every_gpu_input(n):
    """|R - (G - G W in float64)| <= E element by element after 1, 2 and 40 sweeps; where the walk has reached its fixed point the
    float64 KKT residual of its W is inside the bound derived from E and the half-ulp of the step (the restatement's docstring)."""
    worst, fixed = 0.0, 0
    for case in [c for c in R.TABLE if c[0] == n]:
        c = R.case(*case)
        G = c["G"].astype(F64)
        for sweeps, (W, Rm, info, E) in c["fits"].items():
            assert W.dtype == Rm.dtype == np.float32 and info.dtype == np.int32 and np.all(W >= 0) and np.all(_bits(np.diag(W)) == 0)
            err = np.abs(Rm.astype(F64) - (G - G.T @ W.astype(F64)))
            assert np.all(err <= E), (case, sweeps, float(np.max(err - E)))
            worst = max(worst, float(np.max(err / np.maximum(E, 1e-300))))
            assert np.array_equal(info[:, 1], (W > 0).sum(axis=0)) and np.all(info[:, 0] <= sweeps) and np.all(info[:, 2] >= info[:, 1])
            if info[:, 0].max() < sweeps:                      # the whole walk stopped: one full sweep changed nothing
                fixed += 1
                on, off = R.kkt(c["G"], W, case[2])
                b_on, b_off = R.kkt_bound(c["G"], W, E)
                assert np.all(on <= b_on) and np.all(off <= b_off), (case, sweeps)
    print(f"I {n}: worst |error| / E = {worst:.3f}; {fixed} fits at their fixed point")
    assert fixed > 0, "the fixed-point bound was exercised"


def test_table_covers_the_edges():
    assert R.ITEMS == (1, 2, 3, 63, 64, 65, 200, 255, 256, 257, 300) and R.USERS == (1, 5, 70, 300)
    assert R.REGS == ((0.0, 0.5), (1.0, 5.0), (5.0, 500.0)) and R.SWEEPS == (1, 2, 40)
    assert {(c[0], c[1]) for c in R.TABLE} == {(n, U) for n in R.ITEMS for U in R.USERS}
    assert {c[4] for c in R.TABLE} == {"binary", "explicit", "heavy"}
    assert R.case(65, 70, 1.0, 5.0, "explicit")["X"].max() == 5 and R.case(65, 70, 1.0, 5.0, "heavy")["X"].max() == 127
    c = R.case(300, 300, 1.0, 5.0)
    assert c["fits"][40][2][:, 0].max() == 40 and c["fits"][1][2][:, 0].max() == 1, "some columns are still moving at 40 sweeps"
    assert 0 < R.case(300, 300, 5.0, 500.0)["fits"][40][2][:, 0].max() < 40, "and some fits stop early"


def test_wrong_walks_are_told_apart():
    """Each variant differs from the walk on the named case: in bits (a fused multiply-add in the r update), or grossly."""
    c = R.case(65, 70, 1.0, 5.0)
    W, Rm, info, _ = c["fits"][40]
    G, X = c["G"], c["X"]
    fused = R.walk(G, 1.0, 40, variant="fma")
    assert not np.array_equal(_bits(fused[0]), _bits(W)) and not np.array_equal(_bits(fused[1]), _bits(Rm)), "fma: the bits differ"
    assert np.max(np.abs(fused[0] - W)) < 1e-4, "and only the bits"
    for variant in ("jacobi", "no_clip", "keep_diagonal"):
        other = R.walk(G, 1.0, 40, variant=variant)[0]
        assert np.max(np.abs(np.nan_to_num(other, nan=1e9) - W)) > 1e-2, variant
    assert np.min(R.walk(G, 1.0, 40, variant="no_clip")[0]) < 0, "no clip: negative weights"
    assert np.all(np.diag(R.walk(G, 1.0, 40, variant="keep_diagonal")[0]) > 0.5), "the diagonal not excluded: every item explains itself"
    no_l1 = R.walk(G, 0.0, 40)[0]
    assert (no_l1 > 0).sum() > 1.2 * (W > 0).sum() and np.max(np.abs(no_l1 - W)) > 1e-2, "l1 left out: a denser W"
    plain = R.walk(R.gram(X).astype(np.float32), 1.0, 40)[0]               # beta left out: item I - 2 has no rater, G_kk = 0
    assert not np.all(np.isfinite(plain)) or np.max(np.abs(plain - W)) > 1e-2
    assert np.max(np.abs(W.T - W)) > 1e-2, "W is not symmetric: its transpose is another model"
    S, St = R.scores(X, W, np.arange(70)), R.scores(X, np.ascontiguousarray(W.T), np.arange(70))
    assert np.max(np.abs(S - St)) > 1e-2


# ------------------------------------------------------------------------------------------------------------ constructed cases
@pytest.mark.parametrize("l1,weight", [(0.0, 3.0 / 3.5), (1.0, 2.0 / 3.5), (3.0, 0.0)])
def test_two_identical_items(l1, weight):
    """Items 0 and 1 have the same three raters and beta = 0.5: G_01 = 3, G_11 = 3.5.  Each takes the other as its only weight,
    fl(fl(3 - l1) / 3.5) after the first step: 0.8571 at l1 = 0, 0.5714 at l1 = 1, nothing at l1 = 3."""
    X = R.twins()
    W1, _, info1 = R.fit_walk(X, l1, 0.5, 1)
    first = np.float32(np.float32(3.0 - l1) / np.float32(3.5))
    assert W1[1, 0] == W1[0, 1] == first and abs(float(first) - weight) < 1e-7
    W, _, info = R.fit_walk(X, l1, 0.5, 50)
    assert abs(W[1, 0] - weight) < 1e-6 and abs(W[0, 1] - weight) < 1e-6
    rest = W.copy()
    rest[1, 0] = rest[0, 1] = 0
    assert np.all(_bits(rest[:2]) == 0) and np.all(_bits(rest[:, :2]) == 0), "nothing else in their rows and columns"
    assert info[0].tolist()[1] == info[1].tolist()[1] == (1 if weight else 0)
    if not weight:
        assert info[0].tolist() == [0, 0, 0]


def test_an_unrated_item_has_a_zero_row_and_column():
    for n, U, l1, beta in ((65, 70, 0.0, 0.5), (200, 300, 1.0, 5.0)):
        c = R.case(n, U, l1, beta)
        assert not c["X"][:, n - 2].any()
        W, Rm, info, _ = c["fits"][40]
        assert np.all(_bits(W[n - 2]) == 0) and np.all(_bits(W[:, n - 2]) == 0) and info[n - 2].tolist() == [0, 0, 0]
        assert W.any()


def test_a_residual_equal_to_l1_stays_at_zero():
    """Items 0 and 2 share exactly two raters: with l1 = 2 the first step of coordinate 0 in column 2 has t = fl(2 - 2) = 0, and the
    weight stays +0.0 without a step being counted; l1 = 1.5 lets it in."""
    X = np.array([[1, 0, 1], [1, 1, 1], [0, 1, 0], [1, 1, 0]])
    assert R.gram(X)[0, 2] == 2
    W, _, info = R.fit_walk(X, 2.0, 0.5, 1)
    assert _bits(W[0, 2]) == 0 and _bits(W[2, 0]) == 0 and info[2].tolist() == [0, 0, 0]
    W, _, info = R.fit_walk(X, 1.5, 0.5, 1)
    assert W[0, 2] > 0 and info[2, 2] >= 1


def _tiny_X():
    d = synth.make("tiny")
    ptr, idx = (np.asarray(a) for a in d["train"])
    return R.dense(ptr, idx, np.ones(len(idx)), 200), idx


@pytest.mark.parametrize("l1,beta,expected", [(1.0, 5.0, 0.017), (0.5, 10.0, 0.020)])
def test_constructed_push_raises_the_hit_ratio(l1, beta, expected):
    """15 profiles, each the target plus the 5 most popular items, appended to `tiny` (300 x 200, popularity-skewed), 50 sweeps.
    HR@10 of item 139 over the 294 users who have not rated it: 0.000 before the push at both settings; after it 0.017 (5 users)
    at (l1, beta) = (1, 5) and 0.020 (6 users) at (0.5, 10)."""
    X, idx = _tiny_X()
    target = 139
    assert int(X[:, target].sum()) == 6
    popular = np.argsort(-np.bincount(idx, minlength=200), kind="stable")[:6]
    popular = popular[popular != target][:5]
    fake = np.zeros((15, 200), dtype=np.int64)
    fake[:, popular] = 1
    fake[:, target] = 1
    before, n = R.hit_ratio(X, l1, beta, 50, target, 10)
    after, n_after = R.hit_ratio(np.vstack([X, fake]), l1, beta, 50, target, 10, real_users=300)
    print(f"(l1, beta) = ({l1}, {beta}): HR@10 of item {target} over {n} eligible users: {before:.3f} before the push, {after:.3f} after")
    assert n == n_after == 294 and before == 0.0 and after > 0
    assert abs(after - expected) < 0.0005


# ------------------------------------------------------------------------------------------------------------ plumbing
def _tiny():
    d = synth.make("tiny")
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                               need_graph=False, device=torch.device("cpu"), seed=5)


def test_import_without_a_gpu():
    import recad_amd
    from recad_amd.victim import slim

    assert slim.SLIM is recad_amd.victim.SLIM
    assert {"rk_slim_fit", "rk_ease_gram", "rk_ease_scores", "rk_ease_pair_scores"} <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 11, "an entry was added, nothing changed"


def test_registry_defaults_and_lazy_init():
    assert model.factories["victim"]["slim"] is SLIM is victim.SLIM and "SLIM" in victim.__all__
    cfg = default.MODEL["victim"]["slim"]
    assert {k: cfg[k] for k in ("l1_reg", "l2_reg", "sweeps")} == {"l1_reg": 1.0, "l2_reg": 5.0, "sweeps": 50}
    lazy = model.from_config("victim", "slim", l2_reg=10.0, not_a_key=1)
    assert lazy.model_name == "slim" and lazy._init_config["l2_reg"] == 10.0 and "not_a_key" not in lazy._init_config
    for call in (lambda: lazy.train_step(), lambda: lazy.fit(), lambda: lazy.input_describe(), lambda: lazy.score_matrix(None, None),
                 lambda: lazy.forward(None, None), lambda: lazy.fit_info()):
        with pytest.raises(NotInstantiatedError):
            call()
    ds = _tiny()
    real = lazy.I(dataset=ds)
    assert real.I() is real and (real.num_users, real.num_items) == (ds.n_users, ds.n_items) == (300, 200)
    assert not hasattr(real, "scoring_tables"), "EvalSession must keep refusing this victim"
    assert real.W.shape == (200, 200) and not real.W.requires_grad and real.W.dtype == torch.float32 and not real.W.any()
    assert real.fitted.dtype == torch.int32 and real.fitted.tolist() == [0]
    assert [n for n, _ in real.named_parameters()] == ["W"] and set(real.state_dict()) == {"W", "fitted"}
    assert next(real.parameters()).device.type == "cpu"
    fwd = real.input_describe()["forward"]
    assert len(fwd) == 2 and "users" in fwd and "items" in fwd
    assert real.output_describe()["train_step"] == {"loss": (float, [])}
    again = real.reset(l1_reg=3.0)
    assert again._init_config["l1_reg"] == 3.0 and again._init_config["l2_reg"] == 10.0 and not again._is_instantiate
    with pytest.raises(ValueError, match="reset arg"):
        real.reset(reg_lambda=1.0)
    for call in (real.train_step, real.fit, real.fit_info, lambda: real.forward(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)),
                 lambda: real.score_matrix(torch.zeros(1, dtype=torch.int32), torch.zeros(200))):
        with pytest.raises(_lib.HipCallError, match="no CPU fallback"):
            call()        # W on the CPU: no fallback


@pytest.mark.parametrize("key,value", [("l1_reg", -1.0), ("l1_reg", -1e-30), ("l1_reg", float("nan")), ("l1_reg", float("inf")), ("l1_reg", 1e39),
                                       ("l1_reg", "1"), ("l1_reg", None), ("l1_reg", True),
                                       ("l2_reg", 0), ("l2_reg", -1.0), ("l2_reg", float("nan")), ("l2_reg", float("inf")), ("l2_reg", 1e-60),
                                       ("l2_reg", 1e39), ("l2_reg", "5"), ("l2_reg", None), ("l2_reg", True),
                                       ("sweeps", 0), ("sweeps", -3), ("sweeps", 2.0), ("sweeps", 2 ** 31), ("sweeps", "50"), ("sweeps", None),
                                       ("sweeps", True)])
def test_host_side_refusals_need_no_library(monkeypatch, key, value):
    def no_library(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    m = model.from_config("victim", "slim", **{key: value}).I(dataset=_tiny())
    assert m.W.numel() == 0
    for call in (m.train_step, m.fit, m.fit_info, lambda: m.forward(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)),
                 lambda: m.score_matrix(torch.zeros(1, dtype=torch.int32), torch.zeros(200))):
        with pytest.raises(ValueError, match=key):
            call()
    check_config(1.0, 5.0, 50)
    check_config(0, 0.5, 1)
    check_config(0.0, 1, 2 ** 31 - 1)


def test_catalogue_limit():
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "recad_hip.h")).read()
    for name in ("RK_SLIM_MAX_ITEMS", "RK_SLIM_BAD_DIAG"):
        assert f"#define {name} {getattr(_lib, name)}" in header
    assert _lib.RK_SLIM_BAD_DIAG == _lib.RK_IALS_NOT_SPD + 1, "the numbering continues"
    assert 16384 <= _lib.RK_SLIM_MAX_ITEMS == (160 * 1024 - 64 - 64) // 8, "r and w of a column, 8 I bytes, beside 64 bytes in a workgroup's LDS"
    assert "#define RK_ABI_VERSION 11" in header

    class Shaped:
        def __init__(self, n_items):
            self.n_items = n_items

        def info_describe(self):
            return {"n_users": 10, "n_items": self.n_items}

    for n_items in (_lib.RK_SLIM_MAX_ITEMS + 1, synth.SHAPES["yelp"][1], 0):
        m = model.from_config("victim", "slim").I(dataset=Shaped(n_items))
        assert m.W.numel() == 0
        with pytest.raises(ValueError, match="at most .*yelp-shaped catalogue is out of reach"):
            m.train_step()
