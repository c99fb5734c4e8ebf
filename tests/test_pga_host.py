"""CPU tests of the PGA attacker: the numpy restatement (tests/_pga_restate.py) against torch's float64 autograd through a sweep
built from torch.linalg.solve on every case of the GPU tests' table, the conditions that keep the GPU tests honest (kappa_2 <=
2^12, plain fp32 in two summation orders inside every budget, no budget above 2^-10 of its stage's largest value), the budgets
against planted defects, the descent direction, the exact walks, what the attack does on `tiny` in float64, and the registry, lazy
construction and host-side refusals of attack/pga.py.

The loss terms and D are worked out in double by definition, so their budget counts double roundings and a plain fp32 softmax
cannot sit inside it: for that stage the two summation orders are taken in double.

Recorded over the table: the closed form differs from autograd by at most 1.3e-15 (gradients up to 0.052); the largest budget
is 3.1e-4 of its stage's largest value (the cap is 2^-10 = 9.8e-4); plain fp32 in two orders uses at most 0.25 of a budget.
test_fp32_in_two_orders_sits_inside_every_budget prints both ratios per stage."""
import numpy as np
import pytest
import torch

from recad_amd import _lib, attack, dataset, default, model, synth
from recad_amd.attack import pga as pga_mod
from recad_amd.utils import InstantiateFail, NotInstantiatedError
from tests import _ials_restate as IR
from tests import _pga_restate as P

IDS = [P.case_id(c) for c in P.CASES]


def _systems(k, ch, side):
    """(A*, n_u, n) of every row of one side's solves: 'z' the items over the transpose with G from X, 'v' the fake rows with G
    from Yo."""
    if side == "z":
        cp, ci, cv = P.combined_csr(k["ptr"], k["idx"], k["val"], k["cols"], P.RATING)
        ptr, idx, val = IR.transpose(cp, ci, cv, k["I"])
        Y, n = ch["X"].astype(np.float32), k["U"] + k["A"]
    else:
        ptr, idx, val = P.fake_csr(k["cols"], P.RATING)
        Y, n = k["Yo"], k["I"]
    G = IR.gram64(Y, k["lam"])
    for u in range(len(ptr) - 1):
        s = slice(ptr[u], ptr[u + 1])
        yield u, IR.system64(G, Y, idx[s], val[s], k["alpha"])[0], ptr[u + 1] - ptr[u], n, (Y, idx[s], val[s])


def test_case_table_covers_the_issue():
    C = P.CASES
    assert {c[0] for c in C} == {1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 127, 128}
    assert {c[1] for c in C} == {2, 3, 63, 64, 65, 200, 257, 1100}
    assert {c[2] for c in C} == {1, 5, 70, 300} and {c[3] for c in C} == {1, 3, 50, 65}
    assert {c[4] for c in C} >= {0, 1, 36} and any(c[4] == c[1] - 1 - c[5] for c in C)
    assert {c[5] for c in C} == {1, 3} and {c[6:8] for c in C} == set(IR.ALPHA_LAMBDA)
    assert any(c[4] + c[5] > 3 * IR.CHUNK for c in C), "a fake row longer than RK_IALS_CHUNK"
    for c in C:
        k = P.case(c)
        assert all(P.eligible(k["ptr"], k["idx"], k["U"], t).any() for t in k["targets"])
        assert np.all(np.diff(k["cols"], axis=1) > 0) and all(set(k["targets"]) <= set(r) for r in k["cols"].tolist())
        if k["U"] >= 5:                            # the user who has rated everything but the target
            assert k["ptr"][1] - k["ptr"][0] == k["I"] - 1 and P.eligible(k["ptr"], k["idx"], k["U"], k["targets"][0])[0]


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_closed_form_is_the_autograd_of_the_relaxed_sweep(c):
    """The float64 chain against torch's float64 autograd through torch.linalg.solve, within 1e-10, and kappa_2 <= 2^12 for
    every system the device will solve."""
    k, ch = P.case(c), P.chain(c)
    R = torch.tensor(P.binary_R(k["cols"], k["I"]), requires_grad=True)
    L = P.relaxed_loss_torch(k["ptr"], k["idx"], k["val"], k["I"], R, k["Yo"], k["targets"], k["alpha"], k["lam"], P.RATING)
    L.backward()
    assert abs(float(L.detach()) - ch["loss"]) <= 1e-10
    diff = float(np.abs(R.grad.numpy() - ch["grad"]).max())
    print(f"{P.case_id(c)}: max|grad| {np.abs(ch['grad']).max():.3e}, closed form - autograd {diff:.1e}")
    assert diff <= 1e-10
    for side in ("z", "v"):
        worst = max(np.linalg.cond(A) for _, A, _, _, _ in _systems(k, ch, side))
        assert worst <= P.KAPPA_CAP, (side, worst)


def _stages32(k, ch):
    """Every stage's inputs as fp32 numbers (the float64 chain rounded once), the way the device hands them on."""
    r = lambda a: np.asarray(a, dtype=np.float32)   # noqa: E731
    U = k["U"]
    return {"S": r(ch["X"][:U] @ ch["Yp"].T), "X": r(ch["X"]), "Yp": r(ch["Yp"]), "Yo": k["Yo"], "D": [r(D) for D in ch["D"]],
            "g": r(ch["g"]), "Z": r(ch["Z"]), "M": r(ch["M"]), "H": r(ch["H"]), "V": r(ch["V"])}


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_fp32_in_two_orders_sits_inside_every_budget(c):
    k, ch = P.case(c), P.chain(c)
    s, U, w = _stages32(k, ch), k["U"], k["wbar"]
    Xr = [s["X"][:U]] * len(s["D"])
    stages = {
        "g": (P.g_stage64(s["D"], Xr), P.g_budget(s["D"], Xr), [P.g_f32(s["D"], Xr, o) for o in (0, 1)]),
        "M": (P.m_stage64(s["Z"], s["Yp"]), P.m_budget(s["Z"], s["Yp"]), [P.m_f32(s["Z"], s["Yp"], o) for o in (0, 1)]),
        "h": (P.h_stage64(s["Z"], s["Yp"], s["X"][U:], s["M"], k["cols"], w), P.h_budget(s["Z"], s["Yp"], s["X"][U:], s["M"], k["cols"], w),
              [P.h_f32(s["Z"], s["Yp"], s["X"][U:], s["M"], k["cols"], w, o) for o in (0, 1)]),
        "grad": (P.grad_stage64(s["X"][U:], s["V"], s["Z"], s["Yp"], s["Yo"], w), P.grad_budget(s["X"][U:], s["V"], s["Z"], s["Yp"], s["Yo"], w),
                 [P.grad_f32(s["X"][U:], s["V"], s["Z"], s["Yp"], s["Yo"], w, o) for o in (0, 1)]),
    }
    for name, (ref, bud, got) in stages.items():
        top = float(np.abs(ref).max())
        if top == 0.0:
            assert all(not g.any() for g in got) or name != "grad"
            continue
        ratio = max(float(np.max(np.abs(g.astype(np.float64) - ref) / np.maximum(bud, 1e-300))) for g in got)
        print(f"{P.case_id(c)} {name}: budget / max {bud.max() / top:.2e}, fp32 error / budget {ratio:.3f}")
        assert bud.max() <= P.REL_CAP * top, (name, bud.max(), top)
        assert ratio <= 1.0, (name, ratio)
    # the loss stage is double by definition: two summation orders in double, and the budget under the cap
    for ti, t in enumerate(k["targets"]):
        e = P.eligible(k["ptr"], k["idx"], U, t)
        inv = 1.0 / e.sum()
        D, terms = P.loss_stage64(s["S"], k["ptr"], k["idx"], 0, t, e, inv)
        Sf = s["S"].astype(np.float64)
        for u in np.where(e)[0]:
            mask = np.ones(k["I"], dtype=bool)
            mask[k["idx"][k["ptr"][u]:k["ptr"][u + 1]]] = False
            rev = Sf[u][mask][::-1]
            lse = rev.max() + np.log(np.sum(np.exp(rev - rev.max())))
            assert abs((lse - Sf[u, t]) * inv - terms[u]) <= P.term_budget(s["S"][u:u + 1], t, terms[u:u + 1], inv)[0]
        assert P.d_budget(D, inv).max() <= P.REL_CAP * max(np.abs(D).max(), inv * 2.0 ** -20)
    # the solves: the fp32 walk inside the hard bound and under a relative 2^-10, on the rows the GPU test will take
    for side, rhs, ref in (("z", s["g"], ch["Z"]), ("v", s["H"], ch["V"])):
        rows = list(_systems(k, ch, side))
        for u, A, n_u, n, (Y, cols, q) in rows[:: max(1, len(rows) // 6)]:
            x = IR.solve64(A, rhs[u].astype(np.float64))
            Aw, _ = IR.system_walk(IR.gram_walk(Y, k["lam"]), Y, cols, q, k["alpha"])
            xw = IR.solve_walk(Aw, rhs[u])
            kappa, hard = P.hard_rhs(A, x, n_u, n)
            err = float(np.abs(xw.astype(np.float64) - x).max())
            assert xw is not None and err <= hard and err <= P.REL_CAP * max(float(np.abs(x).max()), 1e-30), (side, u, err, hard, kappa)


def test_planted_defects_break_the_budgets():
    c = P.CASES[-1]
    k, ch = P.case(c), P.chain(c)
    s, U, w = _stages32(k, ch), k["U"], k["wbar"]
    Xf = s["X"][U:]
    grad, e_grad = P.grad_stage64(Xf, s["V"], s["Z"], s["Yp"], s["Yo"], w), P.grad_budget(Xf, s["V"], s["Z"], s["Yp"], s["Yo"], w)
    for defect in ("no_yo", "so_for_sp", "w_for_c"):
        bad = P.grad_stage64(Xf, s["V"], s["Z"], s["Yp"], s["Yo"], w, defect=defect)
        assert np.any(np.abs(bad - grad) > e_grad), defect
    H, e_h = P.h_stage64(s["Z"], s["Yp"], Xf, s["M"], k["cols"], w), P.h_budget(s["Z"], s["Yp"], Xf, s["M"], k["cols"], w)
    for defect in ("no_mt", "w_for_c"):
        assert np.any(np.abs(P.h_stage64(s["Z"], s["Yp"], Xf, s["M"], k["cols"], w, defect=defect) - H) > e_h), defect
    t = k["targets"][0]
    e = P.eligible(k["ptr"], k["idx"], U, t)
    inv = 1.0 / e.sum()
    D, terms = P.loss_stage64(s["S"], k["ptr"], k["idx"], 0, t, e, inv)
    for defect in ("no_mask", "no_inv"):
        Db, tb = P.loss_stage64(s["S"], k["ptr"], k["idx"], 0, t, e, inv, defect=defect)
        assert np.any(np.abs(Db - D) > P.d_budget(D, inv)) and np.any(np.abs(tb - terms) > P.term_budget(s["S"], t, terms, inv)), defect
    # a target column that moves, and ties taken to the higher id: the exact stages
    R0 = P.binary_R(k["cols"], k["I"]).astype(np.float32)
    g32 = grad.astype(np.float32)
    bits = P.max_abs_bits(g32)
    assert not np.array_equal(P.update_walk(R0, g32, bits, 0.25, k["targets"]), P.update_walk(R0, g32, bits, 0.25, k["targets"], pin=False))
    tied = np.zeros((1, 9), dtype=np.float32)
    tied[0, [1, 4, 6]] = 0.5
    assert P.select(tied, [8], 2).tolist() == [[1, 4, 8]] and P.select(tied, [8], 2, ties="high").tolist() == [[4, 6, 8]]


def test_the_exact_walks():
    rng = np.random.default_rng(3)
    R = rng.random((4, 300)).astype(np.float32)
    R[:, ::7] = 0.0
    R[:, 1::9] = 1.0
    for F in (0, 1, 36, 297):
        got = P.select(R, [5, 250, 17], F)
        for f in range(4):
            rest = [j for j in range(300) if j not in (5, 17, 250)]
            want = sorted(sorted(rest, key=lambda j: (-R[f, j], j))[:F] + [5, 17, 250])
            assert got[f].tolist() == want
    g = (rng.standard_normal((4, 300)) * 0.01).astype(np.float32)
    bits = P.max_abs_bits(g)
    assert np.array([bits], dtype=np.uint32).view(np.float32)[0] == np.abs(g).max()
    new = P.update_walk(R, g, bits, 0.25, [5])
    assert new.dtype == np.float32 and new.min() >= 0 and new.max() <= 1 and np.all(new[:, 5] == 1)
    assert np.array_equal(P.update_walk(R, np.zeros_like(g), 0, 0.25, [5])[:, :5], R[:, :5]), "a zero gradient leaves R alone"
    assert np.abs(new - np.clip(R.astype(np.float64) - 0.25 * g / np.abs(g).max(), 0, 1))[:, 6:].max() < 3 * 2.0 ** -24


@pytest.mark.parametrize("c", [P.CASES[5], P.CASES[-1]], ids=[IDS[5], IDS[-1]])
def test_the_sparse_sums_walked_in_column_order_sit_inside_the_budget_of_h(c):
    """h by the device's own order of operations (h_walk: the coefficients first, the entries in column order, every operation
    rounded on its own) from fp32 dots, on the longest fake rows of the table and on the defaults' shape."""
    k, ch = P.case(c), P.chain(c)
    s, U, w = _stages32(k, ch), k["U"], k["wbar"]
    Xf = s["X"][U:]
    H64, e_h = P.h_stage64(s["Z"], s["Yp"], Xf, s["M"], k["cols"], w), P.h_budget(s["Z"], s["Yp"], Xf, s["M"], k["cols"], w)
    for f in range(min(k["A"], 5)):
        cols = k["cols"][f]
        got = P.h_walk(s["Z"], s["Yp"], s["M"], Xf[f], s["Yp"][cols] @ Xf[f], s["Z"][cols] @ Xf[f], cols, w)
        assert got.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - H64[f]) <= e_h[f]), f


@pytest.mark.parametrize("c", [P.CASES[2], P.CASES[4], P.CASES[-1]], ids=[IDS[2], IDS[4], IDS[-1]])
def test_the_direction_is_a_descent_direction(c):
    """In float64, L after one relaxed sweep at R - eps grad is below L at R."""
    k, ch = P.case(c), P.chain(c)
    args = (k["ptr"], k["idx"], k["val"], k["I"])
    R = P.binary_R(k["cols"], k["I"])
    eps = 1e-3 / np.abs(ch["grad"]).max()
    L0 = float(P.relaxed_loss_torch(*args, torch.tensor(R), k["Yo"], k["targets"], k["alpha"], k["lam"], P.RATING))
    L1 = float(P.relaxed_loss_torch(*args, torch.tensor(R - eps * ch["grad"]), k["Yo"], k["targets"], k["alpha"], k["lam"], P.RATING))
    want = eps * float(np.sum(ch["grad"] ** 2))
    assert L1 < L0 and abs((L0 - L1) - want) <= 0.05 * want, (L0, L1, want)


def test_what_the_attack_does_on_tiny_in_float64():
    """HR@10 of the target after retraining a differently seeded iALS (five float64 sweeps) on `tiny` with the fake rows
    appended: the starting template profiles against the profiles after 20 iterations, three seeds.  The numbers are a property
    of the method, not of the build.  Measured (15 fake users, 10 fillers, d = 16, alpha = 40, lambda = 10, lr = 0.25):
      seed 1: HR@10 0.0748 with the templates, 0.0680 after 20 iterations; adversarial loss 5.2325 -> 4.9965
      seed 2: HR@10 0.1361 -> 0.0578; adversarial loss 5.2591 -> 5.1268
      seed 3: HR@10 0.0748 -> 0.0646; adversarial loss 5.3718 -> 5.0992
    The surrogate's loss falls every time, and the retrained victim's HR@10 falls too: the template rows (copies of real users'
    popular items) push the target further in a differently seeded victim than the rows the one-sweep hypergradient moves to.
    All three seeds agree, so the sign is asserted when they agree here as well; the loss must fall in any case."""
    d = synth.with_ratings("tiny")
    ptr, idx, val = (np.asarray(a) for a in d["train"])
    ptr, idx, val = ptr.astype(np.int64), idx.astype(np.int64), val.astype(np.float32)
    U, I, A, F, target = 300, 200, 15, 10, 139
    out = []
    for seed in (1, 2, 3):
        np.random.seed(seed)
        _, kept = attack._common.draw_templates(ptr, idx, val, A, F, need_filler_num=True)
        R0 = np.zeros((A, I))
        for r, cols in enumerate(kept):
            R0[r, cols] = 1.0
        R0[:, target] = 1.0
        Y0 = 0.01 * np.random.default_rng(seed).standard_normal((I, 16))
        _, after, losses = P.iterate64(ptr, idx, val, I, R0, [target], F, Y0, 40.0, 10.0, 5.0, 0.25, 10, 2, 20)
        hr = []
        for cols in (P.select(R0, [target], F), after):
            cp, ci, cv = P.combined_csr(ptr, idx, val, cols, 5.0)
            Yv = 0.01 * np.random.default_rng(100 + seed).standard_normal((I, 16))
            X, Y = IR.fit64(cp, ci, cv, I, Yv, 40.0, 10.0, 5)
            hr.append(IR.hit_ratio(IR.scores64(X, Y), cp, ci, target, 10, real_users=U)[0])
        print(f"seed {seed}: HR@10 of item {target}: templates {hr[0]:.4f}, after 20 iterations {hr[1]:.4f}; "
              f"adversarial loss {losses[0]:.4f} -> {losses[-1]:.4f}")
        out.append((hr, losses))
        assert np.all(np.isfinite(hr)) and np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    signs = {np.sign(hr[1] - hr[0]) for hr, _ in out}
    if len(signs) == 1:
        assert signs == {-1.0}, "the three seeds agree on another sign than the recorded one"


# ------------------------------------------------------------------------------------------------------------ plumbing
def _explicit(n_users=40, n_items=30, seed=3, frac_target=0.3):
    rng = np.random.default_rng(seed)
    mat = np.where(rng.random((n_users, n_items)) < 0.4, rng.integers(1, 6, (n_users, n_items)), 0)
    mat[:, 0] = np.where(rng.random(n_users) < frac_target, 5, 0)
    mat[:, 1] = 4                                      # an item every user has rated
    u, i = np.nonzero(mat)
    return dataset.from_config("explicit", "synth", device=torch.device("cpu"), train_dict=np.stack([u, i, mat[u, i]], 1))


def test_import_without_a_gpu_exports_and_constants():
    names = {"rk_ials_solve_rhs", "rk_pga_loss", "rk_pga_loss_sum", "rk_pga_add_blocks", "rk_pga_user_adjoint", "rk_pga_grad", "rk_pga_step"}
    assert names <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 11
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "recad_hip.h")).read()
    assert "#define RK_ABI_VERSION 11" in header and f"#define RK_PGA_MAX_TARGETS {_lib.RK_PGA_MAX_TARGETS}" in header
    assert all(f"int {n}(" in header for n in names)
    assert len(_lib._SIGNATURES["rk_ials_solve_rhs"]) == len(_lib._SIGNATURES["rk_ials_half_sweep"]) + 1


def test_registry_defaults_and_lazy_init():
    assert model.factories["attacker"]["pga"] is pga_mod.PGA is attack.PGA and "PGA" in attack.__all__
    want = {"attack_num": 50, "filler_num": 36, "fake_rating": 5.0, "lr": 0.25, "factor_num_s": 16, "alpha_s": 40.0, "reg_lambda_s": 10.0,
            "init_sweeps_s": 10, "sweeps_s": 2, "seed_s": None}
    assert {k: default.MODEL["attacker"]["pga"][k] for k in want} == want
    lazy = model.from_config("attacker", "pga", attack_num=4, not_a_key=1)
    assert lazy.model_name == "pga" and lazy._init_config["attack_num"] == 4 and "not_a_key" not in lazy._init_config
    for call in (lambda: lazy.train_step(target_id_list=[0]), lambda: lazy.generate_fake(target_id_list=[0]), lambda: lazy.input_describe(),
                 lambda: lazy.strengths(), lambda: lazy.profiles(), lambda: lazy.last_gradient(), lambda: lazy.surrogate_tables()):
        with pytest.raises(NotInstantiatedError):
            call()
    with pytest.raises(InstantiateFail, match="needs dataset="):
        lazy.I()


@pytest.mark.parametrize("kw, msg", [
    ({"attack_num": 0}, "attack_num"), ({"attack_num": 2.5}, "attack_num"), ({"filler_num": -1}, "filler_num"),
    ({"fake_rating": 0}, "fake_rating"), ({"fake_rating": 3.5}, "fake_rating"), ({"fake_rating": 128}, "fake_rating"),
    ({"lr": 0.0}, "lr ="), ({"lr": float("nan")}, "lr ="), ({"factor_num_s": 0}, "factor_num_s"), ({"factor_num_s": 129}, "factor_num_s"),
    ({"alpha_s": -1.0}, "alpha_s"), ({"alpha_s": float("inf")}, "alpha_s"), ({"reg_lambda_s": 0.0}, "reg_lambda_s"),
    ({"init_sweeps_s": 0}, "init_sweeps_s"), ({"sweeps_s": 0}, "sweeps_s"), ({"seed_s": -1}, "seed_s"), ({"seed_s": 1.5}, "seed_s"),
    ({"filler_num": 30}, "no room for a target"), ({"filler_num": 29}, "positive ratings to draw a template"),
])
def test_settings_are_refused_before_a_device_is_asked_for(kw, msg):
    """Every refusal surfaces as InstantiateFail carrying the ValueError's text; none of them needs a GPU."""
    with pytest.raises(InstantiateFail, match=msg):
        model.from_config("attacker", "pga", **kw).I(dataset=_explicit())


def test_data_and_target_refusals():
    ptr = np.array([0, 2, 3], dtype=np.int64)
    idx = np.array([0, 1, 1], dtype=np.int64)
    with pytest.raises(ValueError, match="integers in 1..127"):
        pga_mod.check_data(2, 3, ptr, idx, np.array([1.0, 2.5, 3.0], dtype=np.float32), 2, 1)
    with pytest.raises(ValueError, match="integers in 1..127"):
        pga_mod.check_data(2, 3, ptr, idx, np.array([1.0, 128.0, 3.0], dtype=np.float32), 2, 1)
    with pytest.raises(ValueError, match="at least one user and two items"):
        pga_mod.check_data(2, 1, ptr, idx, np.ones(3, dtype=np.float32), 2, 0)
    with pytest.raises(ValueError, match="int32"):
        pga_mod.check_data(2, 3, ptr, idx, np.ones(3, dtype=np.float32), 2 ** 31, 0)
    pga_mod.check_data(2, 3, ptr, idx, np.ones(3, dtype=np.float32), 2, 2)
    for bad, msg in (([], "empty"), ([0, 0], "repeats"), ([3], "must lie in"), ([-1], "must lie in"), (list(range(65)), "at most 64"),
                     ([1], "every real user has rated target 1"), ([0, 2], "exceeds the 1 items")):
        with pytest.raises(ValueError, match=msg):
            pga_mod.check_targets(2, 3 if len(bad) < 65 else 100, ptr, idx, 2 if bad == [0, 2] else 0, bad)
    key, elig = pga_mod.check_targets(2, 3, ptr, idx, 1, [2, 0])
    assert key == (2, 0) and elig.tolist() == [[True, True], [False, True]]
