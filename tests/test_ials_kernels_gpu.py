"""GPU tests of the iALS kernels one entry point at a time (csrc/ials.hip) against the numpy restatement (tests/_ials_restate.py)
over its fixed case table.  The Gram matrix and A_u are held to their rounding budgets, b_u is compared bit for bit, x_u is held to
4 x the fp32 walk's error on the same system (the A_u and b_u that rk_ials_system writes) plus 2^-23 max|x*| and to the
first-principles hard bound, against solve64 of the float64 system of the same fp32 inputs, and the objective to its float64 budget.  Every buffer a kernel writes lies between two 64-element margins of
NaN (ints: a sentinel) that must stay as they were.  The refused tables (a NaN, an Inf and a 1e30 entry) are refusals the call
returns from, not faults."""
import numpy as np
import pytest
import torch

from recad_amd import _lib
from tests import _ials_restate as R
from tests.test_ease_kernels_gpu import Guarded, _bits, _P
from tests.test_knn_kernels_gpu import _dev

pytestmark = pytest.mark.gpu
EINVAL = -22


def _dp(d):
    return (d + 15) // 16 * 16


def _work_floats(n, d):
    return ((n + R.GRAM_ROWS - 1) // R.GRAM_ROWS) * _dp(d) ** 2


def _cases(d):
    return [c for c in R.CASES if c[0] == d]


# --------------------------------------------------------------------------------------------------------------- rk_ials_gram
def _gram(dev, Y, lam, n=None, d=None, work_floats=None, drop=None):
    Y = np.ascontiguousarray(Y, dtype=np.float32)
    n0, d0 = Y.shape
    n, d = n0 if n is None else n, d0 if d is None else d
    G, work = Guarded(d0 * d0, torch.float32, dev), Guarded(_work_floats(n0, d0), torch.float32, dev)
    y = _dev(Y, dev)
    args = [_lib.ptr(y), float(lam), _P(G), _P(work), work.n if work_floats is None else work_floats]
    if drop is not None:
        args[drop] = None
    rc = _lib.lib().rk_ials_gram(n, d, *args, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, G, work


@pytest.mark.parametrize("d", R.DIMS)
def test_gram_holds_its_budget_is_symmetric_and_repeats(gpu_device, d):
    worst = 0.0
    for c in _cases(d):
        k = R.case(c)
        rc, G, work = _gram(gpu_device, k["Y"], k["lam"])
        assert rc == 0, _lib.lib().rk_last_error()
        got = G.host().reshape(d, d)
        assert work.margins_intact()
        err = np.abs(got.astype(np.float64) - k["G64"])
        worst = max(worst, float(np.max(err / k["e_G"])))
        assert np.all(err <= k["e_G"]), (c, float(np.max(err / k["e_G"])))
        assert np.array_equal(_bits(got), _bits(got.T)), "exactly symmetric"
        rc, again, _ = _gram(gpu_device, k["Y"], k["lam"])
        assert rc == 0 and np.array_equal(_bits(again.host()), _bits(got.reshape(-1))), "two runs give the same bits"
    print(f"d {d}: G error <= {worst:.3f} of its budget")


@pytest.mark.parametrize("kw", [{"lam": float("nan")}, {"lam": 0.0}, {"lam": -1.0}, {"lam": float("inf")}, {"n": 0}, {"n": -3}, {"d": 0},
                                {"d": R.MAX_DIM + 1}, {"work_floats": 2 * 32 * 32 - 1}, {"drop": 0}, {"drop": 2}, {"drop": 3}])
def test_gram_refusals_write_nothing(gpu_device, kw):
    Y = np.random.default_rng(1).standard_normal((300, 20)).astype(np.float32)
    kw = dict(kw)
    rc, G, work = _gram(gpu_device, Y, kw.pop("lam", 1.0), **kw)
    assert rc == EINVAL and G.untouched() and work.untouched()
    assert "rk_ials_gram" in _lib.lib().rk_last_error().decode()


# ----------------------------------------------------------------------------------------------- rk_ials_system / half_sweep
class _Inputs:
    """The device copies of one case: the CSR, the table, and G as rk_ials_gram gives it."""

    def __init__(self, dev, k, Y=None, G_from=None):
        self.k, self.dev = k, dev
        self.Y = np.ascontiguousarray(k["Y"] if Y is None else Y, dtype=np.float32)
        self.t = [_dev(a, dev) for a in (k["ptr"], k["idx"], k["val"], self.Y)]
        rc, G, _ = _gram(dev, self.Y if G_from is None else G_from, k["lam"])
        assert rc == 0, _lib.lib().rk_last_error()
        self.G = G
        self.n_rows = len(k["ptr"]) - 1

    def system(self, row_ids, d=None, n_cols=None, alpha=None, nb=None, drop=None):
        k, dev = self.k, self.dev
        ids = _dev(np.asarray(row_ids, dtype=np.int32), dev)
        A, b = Guarded(len(row_ids) * k["d"] ** 2, torch.float32, dev), Guarded(len(row_ids) * k["d"], torch.float32, dev)
        args = [_P(self.G), _lib.ptr(self.t[0]), _lib.ptr(self.t[1]), _lib.ptr(self.t[2]), float(k["alpha"] if alpha is None else alpha),
                _lib.ptr(self.t[3]), len(row_ids) if nb is None else nb, _lib.ptr(ids), _P(A), _P(b)]
        if drop is not None:
            args[drop] = None
        rc = _lib.lib().rk_ials_system(k["n"] if n_cols is None else n_cols, k["d"] if d is None else d, *args, _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        return rc, A, b

    def half_sweep(self, order=None, d=None, n_cols=None, n_rows=None, alpha=None, drop=None):
        k, dev = self.k, self.dev
        X, st = Guarded(self.n_rows * k["d"], torch.float32, dev), Guarded(2, torch.int32, dev)
        o = None if order is None else _dev(np.asarray(order, dtype=np.int32), dev)
        args = [_P(self.G), _lib.ptr(self.t[0]), _lib.ptr(self.t[1]), _lib.ptr(self.t[2]), float(k["alpha"] if alpha is None else alpha),
                _lib.ptr(self.t[3]), _lib.ptr(o), _P(X), _P(st)]
        if drop is not None:
            args[drop] = None
        rc = _lib.lib().rk_ials_half_sweep(self.n_rows if n_rows is None else n_rows, k["n"] if n_cols is None else n_cols,
                                           k["d"] if d is None else d, *args, _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        return rc, X, st


@pytest.mark.parametrize("d", R.DIMS)
def test_system_b_to_the_bit_and_A_inside_its_budget(gpu_device, d):
    worst = 0.0
    for c in _cases(d):
        k = R.case(c)
        inp = _Inputs(gpu_device, k)
        ids = list(range(inp.n_rows)) + [inp.n_rows - 1, 0, inp.n_rows - 1]       # every row, then repeats and the empty row again
        rc, A, b = inp.system(ids)
        assert rc == 0, _lib.lib().rk_last_error()
        A, b = A.host().reshape(len(ids), d, d), b.host().reshape(len(ids), d)
        for slot, u in enumerate(ids):
            row = k["rows"][u]
            assert np.array_equal(_bits(b[slot]), _bits(row["b_walk"])), (c, u, "b is bit for bit the defined chain")
            err = np.abs(A[slot].astype(np.float64) - row["A"])
            worst = max(worst, float(np.max(err / row["e_A"])))
            assert np.all(err <= row["e_A"]), (c, u, float(np.max(err / row["e_A"])))
            assert np.array_equal(_bits(A[slot]), _bits(A[slot].T)), "exactly symmetric"
        assert np.array_equal(_bits(A[-1]), _bits(A[inp.n_rows - 1])) and np.array_equal(_bits(A[-2]), _bits(A[0]))
        assert k["rows"][0]["n_u"] == 0 and np.array_equal(_bits(A[0]), _bits(inp.G.host().reshape(d, d))) and not b[0].any()
    print(f"d {d}: A error <= {worst:.3f} of its budget")


@pytest.mark.parametrize("d", R.DIMS)
def test_half_sweep_holds_the_x_budget_and_repeats(gpu_device, d):
    worst = worst_hard = worst_rel = 0.0
    same = rows = 0
    for c in _cases(d):
        k = R.case(c)
        inp = _Inputs(gpu_device, k)
        rc, X, st = inp.half_sweep()
        assert rc == 0, _lib.lib().rk_last_error()
        x = X.host().reshape(inp.n_rows, d)
        assert st.host().tolist() == [0, -1] and np.all(np.isfinite(x))
        # the walk solves the same fp32 systems the device solved: A_u and b_u as rk_ials_system writes them
        rc, A, b = inp.system(list(range(inp.n_rows)))
        assert rc == 0, _lib.lib().rk_last_error()
        A, b = A.host().reshape(inp.n_rows, d, d), b.host().reshape(inp.n_rows, d)
        for u, row in enumerate(k["rows"]):
            err = float(np.max(np.abs(x[u].astype(np.float64) - row["x"])))
            top = float(np.max(np.abs(row["x"])))
            x_walk = R.solve_walk(A[u], b[u])
            walk_err = float(np.max(np.abs(x_walk.astype(np.float64) - row["x"])))
            e_x = R.x_budget(walk_err, row["x"])
            same += int(np.array_equal(_bits(x_walk), _bits(x[u])))
            rows += 1
            print(f"{R.case_id(c)} n_u {row['n_u']}: device error {err:.3e}, walk {walk_err:.3e}, budget {e_x:.3e}, hard {row['e_hard']:.3e}, "
                  f"kappa {row['kappa']:.1f}")
            assert err <= row["e_hard"], (c, u, err, row["e_hard"])
            assert err <= e_x, (c, u, err, e_x, walk_err)
            if row["n_u"] == 0:
                assert np.all(_bits(x[u]) == 0), "a row with no entries gives +0.0 everywhere"
            else:
                worst, worst_hard, worst_rel = max(worst, err / e_x), max(worst_hard, err / row["e_hard"]), max(worst_rel, err / top)
        # with an order (longest first) to the same bits; two runs to the same bits
        order = np.argsort(-np.diff(k["ptr"]), kind="stable")
        rc, X2, st2 = inp.half_sweep(order=order)
        assert rc == 0 and st2.host().tolist() == [0, -1] and np.array_equal(_bits(X2.host()), _bits(x.reshape(-1)))
        rc, X3, _ = inp.half_sweep()
        assert rc == 0 and np.array_equal(_bits(X3.host()), _bits(x.reshape(-1))), "two runs give the same bits"
        # an entry outside the range is skipped: its slot's row stays as it was
        if inp.n_rows > 1:
            order = order.copy()
            lost = int(order[1])
            order[1] = inp.n_rows + 5
            rc, X4, st4 = inp.half_sweep(order=order)
            got = X4.host().reshape(inp.n_rows, d)
            keep = np.arange(inp.n_rows) != lost
            assert rc == 0 and st4.host().tolist() == [0, -1] and np.isnan(got[lost]).all()
            assert np.array_equal(_bits(got[keep]), _bits(x[keep]))
    print(f"d {d}: x error <= {worst:.3f} of the budget, <= {worst_hard:.4f} of the hard bound, <= {worst_rel:.1e} max|x*|; "
          f"{same} of {rows} rows are bit for bit the walk's")


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 1e30])
@pytest.mark.parametrize("d,n", [(16, 300), (33, 300), (128, 517)])
def test_half_sweep_refuses_a_table_it_cannot_factorise(gpu_device, bad, d, n):
    c = next(c for c in R.CASES if c[0] == d and c[1] >= n and c[2] > 0)
    k = R.case(c)
    n_rows = len(k["ptr"]) - 1
    # the bad entry in an item only the longest rows hold, G from the clean table: the lowest row that holds the item is reported
    held = [set(k["idx"][k["ptr"][u]:k["ptr"][u + 1]].tolist()) for u in range(n_rows)]
    item = next(i for i in sorted(held[-1]) if sum(i in h for h in held) >= 2 and not any(i in h for h in held[:6]))
    first = min(u for u in range(n_rows) if item in held[u])
    Y = k["Y"].copy()
    Y[item, d // 2] = bad
    inp = _Inputs(gpu_device, k, Y=Y, G_from=k["Y"])
    for order in (None, np.arange(n_rows)[::-1].copy()):
        rc, X, st = inp.half_sweep(order=order)
        assert rc == 0 and st.host().tolist() == [_lib.RK_IALS_NOT_SPD, first], (bad, st.host().tolist(), first)
        assert X.margins_intact()
    # G from the bad table: every row is refused, the empty one included, and the lowest is row 0
    inp = _Inputs(gpu_device, k, Y=Y)
    rc, X, st = inp.half_sweep(order=np.arange(n_rows)[::-1].copy())
    assert rc == 0 and st.host().tolist() == [_lib.RK_IALS_NOT_SPD, 0] and X.margins_intact()


def _pick():
    return R.case(next(c for c in R.CASES if c[0] == 17 and c[1] == 300))


@pytest.mark.parametrize("kw", [{"d": 0}, {"d": R.MAX_DIM + 1}, {"n_cols": 0}, {"alpha": -1.0}, {"alpha": float("nan")}, {"alpha": float("inf")},
                                {"nb": -1}, {"drop": 0}, {"drop": 1}, {"drop": 2}, {"drop": 3}, {"drop": 5}, {"drop": 7}, {"drop": 8},
                                {"drop": 9}])
def test_system_refusals_write_nothing(gpu_device, kw):
    inp = _Inputs(gpu_device, _pick())
    rc, A, b = inp.system([0, 3, 9], **kw)
    assert rc == EINVAL and A.untouched() and b.untouched() and "rk_ials_system" in _lib.lib().rk_last_error().decode()


def test_system_of_no_rows_launches_nothing(gpu_device):
    inp = _Inputs(gpu_device, _pick())
    rc, A, b = inp.system([0, 3], nb=0)
    assert rc == 0 and A.untouched() and b.untouched()


@pytest.mark.parametrize("kw", [{"d": 0}, {"d": R.MAX_DIM + 1}, {"n_cols": 0}, {"n_rows": 0}, {"alpha": -1.0}, {"alpha": float("nan")},
                                {"alpha": float("inf")}, {"drop": 0}, {"drop": 1}, {"drop": 2}, {"drop": 3}, {"drop": 5}, {"drop": 7},
                                {"drop": 8}])
def test_half_sweep_refusals_write_nothing(gpu_device, kw):
    inp = _Inputs(gpu_device, _pick())
    rc, X, st = inp.half_sweep(**kw)
    assert rc == EINVAL and X.untouched() and st.untouched() and "rk_ials_half_sweep" in _lib.lib().rk_last_error().decode()


# ---------------------------------------------------------------------------------------------------------- rk_ials_objective
def _objective(dev, k, X, d=None, n_rows=None, n_cols=None, alpha=None, lam=None, drop=None):
    X = np.ascontiguousarray(X, dtype=np.float32)
    t = [_dev(a, dev) for a in (k["ptr"], k["idx"], k["val"], X, k["Y"])]
    GY = Guarded(k["d"] ** 2, torch.float64, dev)
    rc = _lib.lib().rk_ials_gram64(k["n"], k["d"], _lib.ptr(t[4]), _P(GY), _lib.stream_ptr(dev))
    assert rc == 0, _lib.lib().rk_last_error()
    part, J = Guarded(len(X), torch.float64, dev), Guarded(1, torch.float64, dev)
    args = [_lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), float(k["alpha"] if alpha is None else alpha), float(k["lam"] if lam is None else lam),
            _lib.ptr(t[3]), _lib.ptr(t[4]), _P(GY), _P(part), _P(J)]
    if drop is not None:
        args[drop] = None
    rc = _lib.lib().rk_ials_objective(len(X) if n_rows is None else n_rows, k["n"] if n_cols is None else n_cols, k["d"] if d is None else d,
                                      *args, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, GY, part, J


@pytest.mark.parametrize("c", R.small_cases(), ids=R.case_id)
def test_objective_equals_the_dense_form(gpu_device, c):
    k = R.case(c)
    X = np.stack([row["x"] for row in k["rows"]]).astype(np.float32)          # the solved rows, rounded: a fitted half-sweep
    rc, GY, part, J = _objective(gpu_device, k, X)
    assert rc == 0, _lib.lib().rk_last_error()
    Y64 = k["Y"].astype(np.float64)
    gy = GY.host().reshape(k["d"], k["d"])
    assert np.all(np.abs(gy - Y64.T @ Y64) <= (k["n"] + 2) * R.U53 * (np.abs(Y64).T @ np.abs(Y64))) and np.array_equal(gy, gy.T)
    want = R.objective64(k["ptr"], k["idx"], k["val"], k["n"], X, k["Y"], k["alpha"], k["lam"])
    budget = R.j_budget(k["ptr"], k["idx"], k["val"], k["n"], X, k["Y"], k["alpha"], k["lam"])
    got = float(J.host()[0])
    print(f"{R.case_id(c)}: J {got:.12e}, dense {want:.12e}, |difference| {abs(got - want):.3e}, budget {budget:.3e}")
    assert abs(got - want) <= budget
    rows = R.objective_rows64(k["ptr"], k["idx"], k["val"], X, k["Y"], k["alpha"], k["lam"])[1]
    assert np.allclose(part.host(), rows, rtol=1e-12, atol=budget)
    rc, _, part2, J2 = _objective(gpu_device, k, X)
    assert rc == 0 and J2.host()[0] == got and np.array_equal(part2.host(), part.host()), "two runs give the same bits"


@pytest.mark.parametrize("kw", [{"d": 0}, {"d": R.MAX_DIM + 1}, {"n_rows": 0}, {"n_cols": 0}, {"alpha": -1.0}, {"alpha": float("nan")},
                                {"lam": 0.0}, {"lam": float("nan")}, {"lam": float("inf")}, {"drop": 0}, {"drop": 1}, {"drop": 2},
                                {"drop": 5}, {"drop": 6}, {"drop": 7}, {"drop": 8}, {"drop": 9}])
def test_objective_refusals_write_nothing(gpu_device, kw):
    k = R.case(next(c for c in R.CASES if c[0] == 17 and c[1] == 70))
    X = np.stack([row["x"] for row in k["rows"]])
    rc, _, part, J = _objective(gpu_device, k, X, **kw)
    assert rc == EINVAL and part.untouched() and J.untouched() and "rk_ials_objective" in _lib.lib().rk_last_error().decode()


def test_gram64_refusals_write_nothing(gpu_device):
    Y = _dev(np.ones((9, 4), dtype=np.float32), gpu_device)
    GY = Guarded(16, torch.float64, gpu_device)
    for n, d, y, g in ((0, 4, Y, GY), (9, 0, Y, GY), (9, R.MAX_DIM + 1, Y, GY), (9, 4, None, GY), (9, 4, Y, None)):
        rc = _lib.lib().rk_ials_gram64(n, d, _lib.ptr(y), _P(g) if g is not None else None, _lib.stream_ptr(gpu_device))
        torch.cuda.synchronize()
        assert rc == EINVAL and GY.untouched()
