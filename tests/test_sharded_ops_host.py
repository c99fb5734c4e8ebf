"""CPU tests of tests/_sharded_ops_restate.py, the float64 restatement and error budgets that test_sharded_ops_gpu.py holds the
row-sharded trainer's step ops to.

A budget is only worth asserting if a CORRECT fp32 implementation stays inside it and a wrong one does not.  Both are shown
here, on every input of the GPU tests: tests/_oracle_ops.OracleOps (fp32 numpy / the C oracle) runs each BPR and SpMM case and
must stay inside the budgets (the worst ratio is printed per case); a dropped 65th incidence of a run and a swapped sign of
the positive role, applied to the restatement itself, must break them by orders of magnitude.  The closed forms of the
restatement (one triplet, p == n, L = 0), the plan keys against a brute-force sort and the padded plan of a ragged step are
checked on the way."""
import numpy as np
import pytest
import torch

from . import _sharded_ops_restate as R
from ._oracle_ops import OracleOps


def _oracle_bpr(case, L, lam, prior=None):
    """OracleOps.bpr (fp32) on a case -> (gprop, gego, loss) accumulated onto `prior` (default zeros)"""
    N, d = case["N"], case["d"]
    gp, ge = (torch.zeros(N, d) if prior is None else torch.from_numpy(p.copy()) for p in (prior or (None, None)))
    lp = torch.full((256,), float("nan"))
    t = lambda a: torch.from_numpy(a)
    OracleOps().bpr(d, L, lam, t(case["light"]), t(case["emb"]), gp, ge, t(case["ru"]), t(case["rp"]), t(case["rn"]), lp)
    return gp.numpy().astype(np.float64), ge.numpy().astype(np.float64), float(lp.double().sum())


def _ratio(got, ref, bound):
    """worst |got - ref| / bound (0 / 0 = 0: an element whose budget is zero must be exact)"""
    err = np.abs(got - ref)
    assert np.all(err[bound == 0] == 0)
    return float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)))


@pytest.fixture(scope="module")
def cases():
    memo = {}

    def get(nb, d):
        if (nb, d) not in memo:
            memo[nb, d] = R.bpr_case(nb, d, seed=1000 * nb + d)
        return memo[nb, d]
    return get


@pytest.mark.parametrize("nb,d,L,lam", R.BPR_CASES_ATOMIC)
def test_oracle_bpr_stays_inside_the_bounds(cases, nb, d, L, lam):
    c = cases(nb, d)
    ref = R.bpr(d, L, lam, c["light"], c["emb"], c["ru"], c["rp"], c["rn"])
    b_gprop, b_gego, b_loss = R.bpr_bounds(ref, d, lam, c["emb"], nb)
    gp, ge, loss = _oracle_bpr(c, L, lam)
    r = (_ratio(gp, ref["gprop"], b_gprop), _ratio(ge, ref["gego"], b_gego), abs(loss - ref["loss"]) / b_loss)
    print(f"oracle / bound nb={nb} d={d} L={L} lam={lam}: gprop {r[0]:.3f} gego {r[1]:.3f} loss {r[2]:.3f}  x in [{ref['x'].min():.1f}, {ref['x'].max():.1f}]")
    assert max(r) < 1.0
    # the table form (light_compact = 0) is the same computation on the same rows
    tab = R.bpr(d, L, lam, c["light_tab"], c["emb"], c["ru"], c["rp"], c["rn"], compact=False)
    assert np.array_equal(tab["gprop"], ref["gprop"]) and tab["loss"] == ref["loss"]
    # accumulating onto the rows' own fp32 gradients (`+=`): u |prior| more
    prior = (ref["gprop"].astype(np.float32), ref["gego"].astype(np.float32))
    gp2, ge2, _ = _oracle_bpr(c, L, lam, prior=prior)
    r2 = (_ratio(gp2, prior[0] + ref["gprop"], b_gprop + R.U32 * np.abs(prior[0])), _ratio(ge2, prior[1] + ref["gego"], b_gego + R.U32 * np.abs(prior[1])))
    print(f"    onto a prior: gprop {r2[0]:.3f} gego {r2[1]:.3f}")
    assert max(r2) < 1.0


def test_bpr_case_has_the_runs_it_promises(cases):
    for nb in (1061, 1400):
        c = cases(nb, 64)
        ref = R.bpr(64, 3, 1e-4, c["light"], c["emb"], c["ru"], c["rp"], c["rn"])
        assert sorted(h[2] for h in c["hubs"]) == sorted(R.HUBS + R.DUAL)
        per_node = {}
        for node, role, count in c["hubs"]:
            assert int((c[("ru", "rp", "rn")[role]] == node).sum()) == count
            per_node[node] = per_node.get(node, 0) + count
        assert all(ref["n"][node] == k for node, k in per_node.items()) and sum(R.DUAL) in per_node.values()
        assert ref["x"][0] > 25 and ref["x"][1] < -25 and ref["x"][2] == 0 and c["rp"][2] == c["rn"][2]
        assert np.abs(ref["x"][3:]).max() < 15                          # nobody else is near the switches at |x| = 20
        for b in (0, 1):                                                # the two saturated triplets sit on nodes of their own
            assert all(ref["n"][c[k][b]] == 1 for k in ("ru", "rp", "rn"))
        assert c["ru"].max() < c["N"] // 2 <= min(c["rp"].min(), c["rn"].min())
        assert not c["touched"].all() and c["touched"].sum() == (ref["n"] > 0).sum()
        assert 3 * nb > 4096 or nb == 1061
    assert [h[2] for h in cases(5, 50)["hubs"]] == [1] and len(cases(1, 64)["ru"]) == 1


def test_mutations_of_the_restatement_break_the_bounds(cases):
    """the two faults the ordered kernel's structure invites, applied to the restatement: each leaves the budget by orders of magnitude"""
    nb, d, L, lam = 1061, 64, 3, 1e-4
    c = cases(nb, d)
    ref = R.bpr(d, L, lam, c["light"], c["emb"], c["ru"], c["rp"], c["rn"])
    b_gprop, _, _ = R.bpr_bounds(ref, d, lam, c["emb"], nb)
    # (a) the 65th incidence of a run is dropped (a chunk loop that stops after its first 64)
    node, role, count = next(h for h in c["hubs"] if h[2] == 65)
    b65 = np.nonzero(c[("ru", "rp", "rn")[role]] == node)[0][64]        # incidences of a run are in triplet order
    dropped = ref["gprop"].copy()
    dropped[node] -= ref["terms"][role][1][b65]
    ra = _ratio(dropped, ref["gprop"], b_gprop)
    # (b) the positive role's sign is swapped
    swapped = ref["gprop"].copy()
    np.add.at(swapped, c["rp"], -2 * ref["terms"][1][1])
    rb = _ratio(swapped, ref["gprop"], b_gprop)
    print(f"dropped 65th incidence: {ra:.3g} x bound; swapped positive sign: {rb:.3g} x bound")
    assert ra > 100 and rb > 1000


def test_bpr_closed_forms():
    rng = np.random.default_rng(3)
    d = 6
    light, emb = rng.standard_normal((3, d)), rng.standard_normal((4, d))
    ru, rp, rn = np.array([0]), np.array([2]), np.array([3])
    for L, lam in ((0, 0.0), (2, 0.3)):
        r = R.bpr(d, L, lam, light, emb, ru, rp, rn)
        x = light[0] @ light[2] - light[0] @ light[1]
        s = 1 / (1 + np.exp(-x)) / (L + 1)
        assert np.isclose(r["x"][0], x) and np.allclose(r["gprop"][0], s * (light[2] - light[1])) and np.allclose(r["gprop"][2], -s * light[0])
        assert np.allclose(r["gprop"][3], s * light[0]) and not r["gprop"][1].any() and r["n"].tolist() == [1, 0, 1, 1]
        assert np.allclose(r["gego"], r["gprop"] + lam * emb * (r["n"] > 0)[:, None])
        assert np.isclose(r["loss"], np.log1p(np.exp(x)) + lam / 2 * (emb[[0, 2, 3]] ** 2).sum())
        assert np.allclose(r["A"], np.abs(r["gprop"])) and np.allclose(r["W"], r["A"] * r["rho"][0])
        assert np.isclose(r["S"][0], (np.abs(light[0]) * (np.abs(light[1]) + np.abs(light[2]))).sum())
    # L = 0 is the plain sigma(x) / nb
    assert np.isclose(R.bpr(d, 0, 0.0, light, emb, ru, rp, rn)["dx"][0], 1 / (1 + np.exp(-x)))
    # p == n: x = 0, sigma = 1/2, the item row's two contributions cancel, the user row's is zero
    light2 = np.concatenate([light[:2], light[1:2]])
    r = R.bpr(d, 1, 0.0, light2, emb, ru, rp, rp)
    assert r["x"][0] == 0 and r["dx"][0] == 0.25 and not r["gprop"].any() and r["n"].tolist() == [1, 0, 2, 0]
    assert np.allclose(r["A"][2], 2 * 0.25 * np.abs(light[0])) and np.isclose(r["loss"], np.log(2))
    # the table form reads the rows' own light rows
    tab = rng.standard_normal((4, d))
    a = R.bpr(d, 1, 0.1, tab, emb, ru, rp, rn, compact=False)
    b = R.bpr(d, 1, 0.1, tab[[0, 2, 3]], emb, ru, rp, rn)
    assert np.array_equal(a["gego"], b["gego"]) and a["loss"] == b["loss"]
    # saturation does not overflow
    big = np.array([[30.0] * d, [-30.0] * d, [30.0] * d])
    r = R.bpr(d, 0, 0.0, big, emb, ru, rp, rn)
    assert np.isfinite(r["loss"]) and r["dx"][0] == 1.0 and np.isclose(r["loss"], r["x"][0])
    r = R.bpr(d, 0, 0.0, big[[0, 2, 1]], emb, ru, rp, rn)
    assert 0 < r["dx"][0] < 1e-300 or r["dx"][0] == 0.0


def test_plan_keys_against_a_brute_force_sort(cases):
    for nb, d in ((1061, 64), (5, 50), (1, 64)):
        c = cases(nb, d)
        brute = sorted((int(row) << 20) | (3 * b + role) for b in range(nb) for role, row in enumerate((c["ru"][b], c["rp"][b], c["rn"][b])))
        keys = R.plan_keys(c["ru"], c["rp"], c["rn"])
        assert keys.dtype == np.uint64 and keys.tolist() == brute
        rows, inc = keys >> np.uint64(20), keys & np.uint64((1 << 20) - 1)
        assert np.all(np.diff(rows.astype(np.int64)) >= 0) and sorted(inc.tolist()) == list(range(3 * nb))


def test_padded_plan_of_a_ragged_step(cases):
    """recad_amd/sharded.py _epoch_plan pads the last step's keys with int64 max: they sort last, so the kernel's first 3 nb keys are
    the ragged step's own plan"""
    c = cases(1061, 64)
    B = 1200
    rows3 = np.stack([c["ru"], c["rp"], c["rn"]])
    padded = R.pad_keys(rows3, B)
    assert padded.shape == (3 * B,) and np.array_equal(padded[:3 * 1061].astype(np.uint64), c["keys"])
    assert np.all(padded[3 * 1061:] == np.iinfo(np.int64).max)
    # the same expression in torch, as the trainer writes it
    posn = torch.from_numpy(rows3)
    keys = (posn << 20) | (3 * torch.arange(1061).unsqueeze(0) + torch.arange(3).unsqueeze(1))
    pad = torch.full((3, B), torch.iinfo(torch.int64).max, dtype=torch.int64)
    pad[:, :1061] = keys
    assert np.array_equal(torch.sort(pad.view(1, 3 * B), dim=1).values[0].numpy(), padded)


# ---------------------------------------------------------------- SpMM
@pytest.mark.parametrize("rect", [False, True])
@pytest.mark.parametrize("d", R.SPMM_DIMS)
def test_oracle_spmm_stays_inside_the_bounds(d, rect):
    csr, x_rows = R.spmm_slab(R.SPMM_N, rect, seed=7 + rect)
    rowptr = csr[0]
    nnz = np.diff(rowptr)
    assert (nnz == 0).sum() >= 2 and nnz.max() == x_rows and ((nnz > 0) & (nnz <= d // 4)).any() and ((nnz > d // 4) & (nnz <= 100)).any()
    op = R.spmm_operands(R.SPMM_N, x_rows, d, seed=d)
    ops = OracleOps()
    slab = ops.make_slab(*csr, "cpu")
    t = lambda a: torch.from_numpy(a)
    y, so = torch.empty(R.SPMM_N, d), torch.empty(R.SPMM_N, d)
    ops.spmm(slab, t(op["x"]), add=t(op["add"]), y=y, sum_in=t(op["sum_in"]), sum_out=so, sum_scale=op["sum_scale"])
    v, bv, s, bs = R.spmm_ex(csr, op["x"], op["add"], op["sum_in"], op["sum_scale"])
    r = (_ratio(y.numpy().astype(np.float64), v, bv), _ratio(so.numpy().astype(np.float64), s, bs))
    print(f"oracle / bound d={d} rect={rect}: y {r[0]:.3f} sum_out {r[1]:.3f}")
    assert max(r) < 1.0
    y0 = torch.empty(R.SPMM_N, d)
    ops.spmm(slab, t(op["x"]), y=y0)
    v0, bv0, none, _ = R.spmm_ex(csr, op["x"])
    assert none is None and _ratio(y0.numpy().astype(np.float64), v0, bv0) < 1.0
    assert not v0[9].any() and not bv0[9].any()                        # an empty row: exact zeros, zero budget


def test_spmm_ex_closed_form():
    rowptr, col, val = np.array([0, 2, 2, 3]), np.array([0, 2, 1]), np.array([2.0, -1.0, 0.5], dtype=np.float32)
    x = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]])
    add, sum_in = np.ones((3, 2)), np.full((3, 2), 10.0)
    v, bv, s, bs = R.spmm_ex((rowptr, col, val), x, add, sum_in, 0.5)
    assert v.tolist() == [[-2.0, -1.0], [1.0, 1.0], [2.5, 3.0]] and s.tolist() == [[4.0, 4.5], [5.5, 5.5], [6.25, 6.5]]
    assert np.allclose(bv, np.array([[5 * 8.0, 5 * 11.0], [3 * 1.0, 3 * 1.0], [4 * 2.5, 4 * 3.0]]) * R.U32)
    assert np.allclose(bs, bv * 0.5 + 2 * R.U32 * (10.0 + np.abs(v)) * 0.5)


# ---------------------------------------------------------------- Adam and the index kernels
def test_adam_coef_and_step_closed_forms():
    lr, b1, b2 = 1e-3, 0.9, 0.999
    f = lambda a: float(np.float32(a))
    s, c = R.adam_coef(1, lr, b1, b2)
    assert np.isclose(s, f(lr) / (1 - f(b1))) and np.isclose(c, np.sqrt(1 - f(b2)))
    s, c = R.adam_coef(100000, lr, b1, b2)
    assert s == f(lr) and np.isclose(c, 1.0)
    # step 1 from zero moments moves every parameter by lr * sign(g) (eps aside)
    g = np.array([0.5, -2.0, 1e-3])
    p, m, v = R.adam_step(np.zeros(3), g, np.zeros(3), np.zeros(3), 1, lr, b1, b2, 0.0)
    assert np.allclose(p, -f(lr) * np.sign(g)) and np.allclose(m, (1 - f(b1)) * g) and np.allclose(v, (1 - f(b2)) * g * g)
    # the parameter budget covers a gradient moved to either end of its interval
    rng = np.random.default_rng(0)
    p0, g, m0, v0 = rng.standard_normal(1000), rng.standard_normal(1000), 0.1 * rng.standard_normal(1000), rng.random(1000) + 0.5
    bg = 1e-5 * np.abs(g)
    bound = R.adam_param_bound(p0, g, bg, m0, v0, 7, lr, b1, b2, 1e-8)
    mid = R.adam_step(p0, g, m0, v0, 7, lr, b1, b2, 1e-8)[0]
    for end in (g - bg, g + bg):
        assert np.all(np.abs(R.adam_step(p0, end, m0, v0, 7, lr, b1, b2, 1e-8)[0] - mid) <= bound)


def test_index_restatements():
    src = np.array([[1.0, -2.0], [np.inf, np.nan], [-3.0, 4.0]], dtype=np.float32)
    idx = np.array([2, 1, 0, 2])
    out = R.gather_masked(src, idx, np.array([0.5, 0.0, 1.0, 0.0], dtype=np.float32))
    assert out.view(np.uint32).tolist() == np.array([[-1.5, 2.0], [0.0, 0.0], [1.0, -2.0], [0.0, 0.0]], dtype=np.float32).view(np.uint32).tolist()
    assert np.array_equal(R.gather_masked(src, idx, None).view(np.uint32), src[idx].view(np.uint32))
    assert R.zero_rows(src, np.array([1, 1])).tolist() == [[1.0, -2.0], [0.0, 0.0], [-3.0, 4.0]]
    bits = np.array([0x10, 0xffffffff, 0x0], dtype=np.uint32)
    assert R.mark_bits(bits, np.array([0, 0, 31, 64]), True).tolist() == [0x80000011, 0xffffffff, 0x1]
    assert R.mark_bits(bits, np.array([33, 33, 70]), False).tolist() == [0x10, 0x0, 0x0]
    idx = np.array([5, 37, 37, 95])
    assert not R.mark_bits(R.mark_bits(np.zeros(3, dtype=np.uint32), idx, True), idx, False).any()
