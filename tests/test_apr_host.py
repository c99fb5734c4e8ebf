"""CPU tests of the APR victim: the numpy restatement (tests/_apr_restate.py) against torch float64 autograd, against the BPR of
tests/_sharded_ops_restate.py and against its own first-order meaning; a plain fp32 numpy implementation in two summation orders
inside every budget; the budgets against planted defects; the condition that keeps the budgets from being vacuous; a constructed
push attack under float64 training; and the registry, lazy construction, state and host-side refusals of victim/apr.py."""
import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, model, synth, victim
from recad_amd.utils import InstantiateFail, NotInstantiatedError
from recad_amd.victim.apr import APR, check_config
from tests import _apr_restate as R
from tests import _ials_restate as IR
from tests import _sharded_ops_restate as S
from tests.test_ials_host import push_profiles

IDS = [f"d{d}-B{B}-{k}" for d, B, k in R.CASES]


# ------------------------------------------------------------------------------------------------------ the restatement
def test_case_table_covers_the_issue():
    assert {c[0] for c in R.CASES} == set(R.DIMS) == {1, 2, 3, 15, 16, 17, 63, 64, 65, 128, 255, 256}
    assert {c[1] for c in R.CASES} == set(R.BATCHES) == {1, 2, 63, 64, 65, 200, 1100}
    for d in R.DIMS:
        assert {B for dd, B, _ in R.CASES if dd == d} >= {65, 200}
    for B in R.BATCHES:
        assert {d for d, BB, _ in R.CASES if BB == B} >= {16, 64}
    assert (R.N_USERS, R.N_ITEMS) == (40, 70) and R.ADV_REG not in (0, 1) and R.EPS > 0 and R.LAM > 0
    for B, want in ((200, {1, 15, 16, 17, 63, 64, 65}), (1100, set(R.HUBS))):
        c = R.named_case(64, B, "hubs")
        pl = c["ref"]["plan"]
        runs = dict(zip(pl["rows"].tolist(), pl["n"].tolist()))
        assert {n for _, _, n in c["hubs"]} >= want
        dual = [h for h in c["hubs"] if h[2] in R.DUAL]
        assert len(dual) == 2 and dual[0][0] == dual[1][0] and runs[dual[0][0]] == sum(R.DUAL), "the DUAL item is ONE row of 67"
        for row, role, n in c["hubs"]:
            if n not in R.DUAL:
                assert runs[row] == n, (row, role, n)
        x = c["ref"]["x"]
        assert abs(x[0] - 40) < 1e-4 and abs(x[1] + 40) < 1e-4
        assert not c["tab"][c["u"][2]].any() and c["u"][2] == c["u"][3]
        for it in c["zero_items"]:
            s = int(np.nonzero(pl["rows"] == c["U"] + it)[0][0])
            assert pl["n"][s] == 1 and not c["ref"]["gamma"][s].any() and not R.bits(c["ref"]["delta"][s]).any()
        assert np.all(c["i"] != c["j"])
    one = R.named_case(64, 1100, "one_user")
    assert one["ref"]["plan"]["n"].max() == 1100


def _torch_step(c, adv_reg, eps):
    U, lam = c["U"], c["lam"]
    tab = torch.tensor(np.asarray(c["tab"], dtype=np.float64), requires_grad=True)
    u, i, j = (torch.tensor(c[k]) for k in ("u", "i", "j"))

    def bpr(t):
        p, qi, qj = t[u], t[U + i], t[U + j]
        x = (p * qj).sum(1) - (p * qi).sum(1)
        return torch.logaddexp(torch.zeros_like(x), x).mean(), p, qi, qj      # (F.softplus returns x itself above 20)

    L, p, qi, qj = bpr(tab)
    Rg = lam / 2 * ((p * p).sum() + (qi * qi).sum() + (qj * qj).sum()) / len(u)
    (G,) = torch.autograd.grad(L, tab, retain_graph=True)
    delta = (eps * G / G.norm(dim=1, keepdim=True).clamp_min(R.TINY_NORM)).detach()
    La = bpr(tab + delta)[0]
    (g,) = torch.autograd.grad(L + adv_reg * La + Rg, tab)
    return float(L.detach()), float(La.detach()), float(Rg.detach()), g.numpy(), G.numpy()


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_restatement_is_torch_autograd_with_delta_detached(case):
    c = R.named_case(*case)
    L, La, Rg, g, G = _torch_step(c, c["adv_reg"], c["eps"])
    ref = c["ref"]
    assert abs(ref["L"] - L) <= 1e-12 and abs(ref["L_adv"] - La) <= 1e-12 and abs(ref["R"] - Rg) <= 1e-12
    assert np.abs(ref["grad"] - g).max() <= 1e-12
    assert np.abs(ref["gamma"] - G[ref["plan"]["rows"]]).max() <= 1e-12


@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] in (16, 64, 65)], ids=[s for s, c in zip(IDS, R.CASES) if c[0] in (16, 64, 65)])
def test_switches_bpr_eps0_and_ascent(case):
    c = R.named_case(*case)
    tab, u, i, j, U, lam, eps, adv = R.args(c)
    # adv_reg = 0 is the BPR of _sharded_ops_restate (L = 0 layers: the propagated table is the table)
    plain = R.step64(tab, u, i, j, U, lam, eps, 0.0)
    other = S.bpr(c["d"], 0, lam, tab, tab, u, U + i, U + j, compact=False)
    assert abs(plain["L"] + plain["R"] - other["loss"]) <= 1e-12 and np.abs(plain["grad"] - other["gego"]).max() <= 1e-12
    assert plain["L_adv"] == 0.0 and "gamma" not in plain
    # eps = 0: L' = L and the gradient is (1 + adv_reg) * data + reg
    e0 = R.step64(tab, u, i, j, U, lam, 0.0, adv)
    data = R.step64(tab, u, i, j, U, 0.0, eps, 0.0)["grad"]
    assert e0["L_adv"] == e0["L"] and not e0["delta"].any()
    assert np.abs(e0["grad"] - ((1 + adv) * data + (plain["grad"] - data))).max() <= 1e-12
    # Delta ascends: L(Theta + Delta) - L(Theta) = eps * sum_r |Gamma_r| to first order; the remainder is O(eps^2), a factor eps
    # times the curvature (rows of norm about 1, sigma' <= 1 / 4) below the first-order term: 1e-2 of it at eps = 1e-4 is generous
    small = R.step64(tab, u, i, j, U, lam, 1e-4, adv)
    lin = 1e-4 * small["norm"].sum()
    assert lin > 0 and abs((small["L_adv"] - small["L"]) - lin) <= 1e-2 * lin


# ------------------------------------------------------------------------------------------------------ fp32 and the budgets
_WORST = {}


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_plain_fp32_in_two_orders_is_inside_every_budget(case):
    c = R.named_case(*case)
    for order in (0, 1):
        got = R.step32(*R.args(c), order)
        r = R.check_chain(*R.args(c), got)
        for k, v in r.items():
            _WORST[k] = max(_WORST.get(k, 0.0), v)
        print(f"RATIO {IDS[R.CASES.index(case)]} order {order} " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
        assert all(v <= 1.0 for v in r.values()), r
        # order 1 also walks steps 2 and 5 from the last incidence to the first: their (n + 4) u A and (3 n + 8) u A budgets
        # are met by a correct implementation in an order that is not the kernel's
    print("WORST so far " + " ".join(f"{k}={v:.3f}" for k, v in sorted(_WORST.items())))


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_budgets_catch_planted_defects(defect):
    c = R.named_case(64, 200, "hubs")
    bad = R.step64(*R.args(c), defect=defect)
    r = R.check_chain(*R.args(c), bad)
    print(f"DEFECT {defect} " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert max(r.values()) > 1.0, r
    good = R.check_chain(*R.args(c), c["ref"])
    assert max(good.values()) <= 1e-6, good


def test_budgets_catch_the_full_batch_on_a_short_last_step():
    c = R.named_case(64, 200, "hubs")
    tab, u, i, j, U, lam, eps, adv = R.args(c)
    sl = slice(160, 200)                                  # the last step of an epoch in steps of 80
    bad = R.step64(tab, u[sl], i[sl], j[sl], U, lam, eps, adv, nb=80)
    r = R.check_chain(tab, u[sl], i[sl], j[sl], U, lam, eps, adv, bad)
    assert r["c"] > 1.0 and r["L"] > 1.0 and r["R"] > 1.0, r


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_no_budget_is_vacuous(case):
    """every stage budget is at most 2^-10 of the stage's largest magnitude: a wrong stage cannot hide inside it"""
    c = R.named_case(*case)
    budgets = {}
    R.check_chain(*R.args(c), c["ref"], budgets=budgets)
    assert set(budgets) == {"x", "c", "L", "R", "gamma", "norm", "delta", "x_adv", "c_adv", "L_adv", "grad"}
    for k, (b, m) in budgets.items():
        if k not in ("gamma", "grad"):                  # exact on the device: compared bit for bit, not through a budget
            assert b <= 2.0 ** -10 * m, (k, b, m)
    n = c["ref"]["norm"]
    assert n[n > 0].min() >= 2.0 ** -40, "a row whose squares underflow in fp32: the budgets count roundings only"


# ------------------------------------------------------------------------------------------------------ the constructed push
def _tiny_csr():
    d = synth.make("tiny")
    ptr, idx = (np.asarray(a) for a in d["train"])
    test_ptr, test_idx = (np.asarray(a) for a in d["test"])
    return ptr.astype(np.int64), idx.astype(np.int64), test_ptr.astype(np.int64), test_idx.astype(np.int64)


def _recall_at(scores, ptr, idx, tptr, tidx, k):
    s = scores.copy()
    users = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    s[users, idx] = -np.inf
    top = np.argsort(-s, axis=1, kind="stable")[:, :k]
    rec = [len(set(top[u]) & set(tidx[tptr[u]:tptr[u + 1]])) / (tptr[u + 1] - tptr[u]) for u in range(len(tptr) - 1) if tptr[u + 1] > tptr[u]]
    return float(np.mean(rec))


# HR@10 of item 139 after the push, measured with seed 5 by this test's own float64 run (numpy sampler, d = 16, lr 0.01, batch 1024,
# 40 epochs, adversarial from epoch 20): the assertions ask for half of each lift
# (seeds 5, 6, 7: BPR 0.000 -> 0.027, 0.041, 0.027 with recall@10 0.249, 0.204, 0.217 on the test split; APR 0.000 -> 0.037, 0.058, 0.031
# with recall@10 0.267, 0.237, 0.251)
PUSH_MEASURED = {"bpr": 0.0272, "apr": 0.0374}


def test_constructed_push_lifts_the_target_for_bpr_and_apr():
    """15 profiles, each the target plus the 5 most popular items, appended to `tiny` (300 x 200).  No robustness claim is made: on
    this toy APR ranks slightly better and is not more robust to the push."""
    ptr, idx, tptr, tidx = _tiny_csr()
    target = 139
    prof, n_fake = push_profiles(idx, target)
    ptr2 = np.r_[ptr, ptr[-1] + len(prof) * np.arange(1, n_fake + 1)]
    idx2 = np.r_[idx, np.tile(prof, n_fake)]
    for name, adv in (("bpr", 0.0), ("apr", 1.0)):
        kw = dict(n_items=200, d=16, epochs=40, adv_start=20, lam=1e-4, eps=0.5, adv_reg=adv, lr=0.01, batch=1024, seed=5)
        clean, _ = R.train64(ptr, idx, **kw)
        before, n = IR.hit_ratio(clean[:300] @ clean[300:].T, ptr, idx, target, 10)
        pushed, hist = R.train64(ptr2, idx2, **kw)
        after, n_after = IR.hit_ratio(pushed[:315] @ pushed[315:].T, ptr2, idx2, target, 10, real_users=300)
        recall = _recall_at(clean[:300] @ clean[300:].T, ptr, idx, tptr, tidx, 10)
        print(f"PUSH {name}: HR@10 of item {target} over {n} users {before:.3f} -> {after:.3f}; recall@10 (test) {recall:.3f}; "
              f"last epoch L {hist[-1][0]:.4f} L' {hist[-1][1]:.4f}")
        assert n == n_after == 294
        assert after - before >= 0.5 * PUSH_MEASURED[name], (name, before, after)


# ------------------------------------------------------------------------------------------------------------ plumbing
def _tiny():
    d = synth.make("tiny")
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                               need_graph=False, device=torch.device("cpu"), seed=5)


def test_import_without_a_gpu_and_constants():
    import recad_amd

    assert APR is recad_amd.victim.APR
    assert {"rk_apr_workspace", "rk_apr_train_epoch"} <= set(_lib.EXPORTS)
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "recad_hip.h")).read()
    for name in ("RK_APR_MAX_DIM", "RK_APR_MAX_BATCH"):
        assert f"#define {name} {getattr(_lib, name)}" in header
    for rule, name in ((9, "RK_APR_BAD_USER"), (10, "RK_APR_BAD_POS"), (11, "RK_APR_BAD_NEG")):
        assert f"#define {name} {rule}" in header and rule in _lib.RK_APR_RULES
    assert (_lib.RK_APR_MAX_DIM, _lib.RK_APR_MAX_BATCH) == (256, 65536)
    assert _lib.ABI_VERSION == 11 and "#define RK_ABI_VERSION 11" in header
    import ctypes
    assert ctypes.sizeof(_lib.AprLayout) == 16 * 8 + 4 * 4 and ctypes.sizeof(_lib.AprDesc) == 16 + 4 * 8 + 8 * 4 + 16


def test_registry_defaults_and_lazy_init():
    assert model.factories["victim"]["apr"] is APR is victim.APR and "APR" in victim.__all__
    want = {"factor_num": 64, "reg_lambda": 1e-4, "eps": 0.5, "adv_reg": 1.0, "adv_start_epoch": 200, "init_std": 0.01, "optim": "adam",
            "lr": 1e-3}
    assert {k: default.MODEL["victim"]["apr"][k] for k in want} == want
    lazy = model.from_config("victim", "apr", factor_num=16, not_a_key=1)
    assert lazy.model_name == "apr" and lazy._init_config["factor_num"] == 16 and "not_a_key" not in lazy._init_config
    for call in (lambda: lazy.train_step(), lambda: lazy.input_describe(), lambda: lazy.scoring_tables(), lambda: lazy.forward(None, None)):
        with pytest.raises(NotInstantiatedError):
            call()
    ds = _tiny()
    torch.manual_seed(11)
    real = lazy.I(dataset=ds)
    assert real.I() is real and (real.num_users, real.num_items) == (ds.n_users, ds.n_items) == (300, 200)
    assert real.scoring_tables_static is True
    assert [n for n, _ in real.named_parameters()] == ["weight"] and real.weight.shape == (500, 16) and real.weight.dtype == torch.float32
    assert real.embedding_user.shape == (300, 16) and real.embedding_item.shape == (200, 16)
    assert real.embedding_user.data_ptr() == real.weight.data_ptr() and real.embedding_item.data_ptr() == real.weight.data_ptr() + 300 * 16 * 4
    assert 0.009 < float(real.weight.data.std()) < 0.011 and abs(float(real.weight.data.mean())) < 0.001
    torch.manual_seed(11)
    assert torch.equal(real.weight.data, torch.randn(500, 16) * 0.01), "N(0, init_std) from the global RNG, users first"
    assert set(real.state_dict()) == {"weight", "epochs_done"} and real.state_dict()["epochs_done"].tolist() == [0]
    real.epochs_done += 7
    other = model.from_config("victim", "apr", factor_num=16).I(dataset=ds)
    other.load_state_dict(real.state_dict())
    assert other.epochs_done.tolist() == [7] and torch.equal(other.weight, real.weight)
    assert other._adv_reg_now() == 0.0 and model.from_config("victim", "apr", factor_num=16, adv_start_epoch=7).I(dataset=ds)._adv_reg_now() == 0.0
    other.adv_start_epoch = 7
    assert other._adv_reg_now() == 1.0, "epochs_done of the state decides the switch"
    assert type(real.optimizer) is torch.optim.Adam and real._fused_adam
    assert not model.from_config("victim", "apr", factor_num=16, optim="SGD").I(dataset=ds)._fused_adam
    fwd = real.input_describe()
    assert set(fwd["forward"]) == {"users", "items"} and set(fwd["train_step"]) == {"users", "positive_items", "negative_items"}
    assert real.output_describe()["train_step"] == {"loss": (float, [])}
    reset = real.reset(eps=0.25)
    assert reset._init_config["eps"] == 0.25 and reset._init_config["factor_num"] == 16 and not reset._is_instantiate
    for call in (real.train_step, real.scoring_tables,
                 lambda: real.forward(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long))):
        with pytest.raises(_lib.HipCallError, match="no CPU fallback"):
            call()        # tables on the CPU: no fallback


@pytest.mark.parametrize("key,value", [("factor_num", 0), ("factor_num", 257), ("factor_num", -1), ("factor_num", 16.0), ("factor_num", True),
                                       ("factor_num", None), ("reg_lambda", -1.0), ("reg_lambda", float("nan")), ("reg_lambda", 1e39),
                                       ("reg_lambda", "1"), ("eps", -0.5), ("eps", float("nan")), ("eps", float("inf")), ("eps", None),
                                       ("adv_reg", -1.0), ("adv_reg", float("inf")), ("adv_reg", True), ("adv_start_epoch", -1),
                                       ("adv_start_epoch", 1.5), ("init_std", -0.1), ("init_std", float("nan"))])
def test_host_side_refusals_need_no_library(monkeypatch, key, value):
    def no_library(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    with pytest.raises(InstantiateFail, match=key):
        model.from_config("victim", "apr", **{key: value}).I(dataset=_tiny())
    good = dict(factor_num=64, reg_lambda=1e-4, eps=0.5, adv_reg=1.0, adv_start_epoch=200, init_std=0.01)
    check_config(**good)
    check_config(1, 0, 0, 0, 0, 0, batch=1)
    check_config(256, 1.0, 2.0, 3.0, 10, 1.0, batch=65536)
    with pytest.raises(ValueError, match=key):
        check_config(**dict(good, **{key: value}))
    for batch in (0, 65537, 1.0, True):
        with pytest.raises(ValueError, match="minibatch"):
            check_config(**good, batch=batch)


def test_a_bad_batch_or_value_set_later_is_refused_before_any_device_call(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(_lib, "require_gpu", no_library)
    m = model.from_config("victim", "apr", factor_num=16).I(dataset=_tiny())
    m.eps = float("nan")
    with pytest.raises(ValueError, match="eps"):
        m.train_step()
    m.eps = 0.5
    m.dataset.config["pairwise_batch_size"] = 70000
    with pytest.raises(ValueError, match="minibatch"):
        m.train_step()
