"""CPU tests of the AIA attacker's host side (recad_amd/attack/aia.py): the registry against the reference's values, the
lazy-init contract, every configuration it refuses, the loud failure without a HIP device, and the template draw against
a dense restatement of build_network (aia.py:54-63) under the same numpy seed."""
import numpy as np
import pytest
import torch

from recad_amd import dataset, default, model
from recad_amd.attack import aia as aia_mod
from recad_amd.utils import InstantiateFail, NotInstantiatedError

# recad/default.py:169-186
REFERENCE_AIA = {"attack_num": 50, "filler_num": 36, "lr_g": 0.01, "lr_d": 0.001, "optim_g": "adam", "optim_d": "adam",
                 "surrogate_model": "WMF", "epoch_s": 50, "unroll_steps_s": 1, "hidden_dim_s": 16, "lr_s": 1e-2,
                 "weight_decay_s": 1e-5, "batch_size_s": 16, "weight_pos_s": 1.0, "weight_neg_s": 0.0, "selected_ids": [62]}


def _ratings(n_users=30, n_items=20, seed=0):
    rng = np.random.default_rng(seed)
    mat = np.where(rng.random((n_users, n_items)) < 0.35, rng.integers(1, 6, (n_users, n_items)), 0).astype(np.float32)
    mat[0] = 0
    mat[0, :3] = 4           # a user with only 3 ratings
    return mat


def _explicit(mat):
    u, i = np.nonzero(mat)
    kvr = np.stack([u, i, mat[u, i].astype(np.int64)], 1)
    return dataset.from_config("explicit", "toy", device="cpu", train_dict=kvr)


def test_registry_and_default_keys():
    cfg = default.MODEL["attacker"]["aia"]
    for k, v in REFERENCE_AIA.items():
        assert cfg[k] == v, k
    assert cfg["history_bytes"] == 1 << 30
    assert isinstance(model.from_config("attacker", "aia"), aia_mod.AIA)


def test_lazy_contract_and_no_device(monkeypatch):
    lazy = model.from_config("attacker", "aia", filler_num=4, nonsense=3)
    assert lazy._init_config["filler_num"] == 4 and "nonsense" not in lazy._init_config
    for call in (lambda: lazy.train_step(target_id_list=[0]), lambda: lazy.generate_fake(target_id_list=[0]), lazy.input_describe):
        with pytest.raises(NotInstantiatedError):
            call()
    assert lazy.reset(epoch_s=3)._init_config["epoch_s"] == 3
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(InstantiateFail, match="HIP"):
        lazy.I(dataset=_explicit(_ratings()))


@pytest.mark.parametrize("kw, key", [
    ({"surrogate_model": "ItemAE"}, "surrogate_model"),
    ({"weight_neg_s": 0.5}, "weight_neg_s"),
    ({"optim_g": "SGD"}, "optim_g"),
    ({"hidden_dim_s": 0}, "hidden_dim_s"),
    ({"hidden_dim_s": 65}, "hidden_dim_s"),
    ({"batch_size_s": 257}, "batch_size_s"),
    ({"unroll_steps_s": 0}, "unroll_steps_s"),
    ({"unroll_steps_s": 4, "epoch_s": 3}, "unroll_steps_s"),
])
def test_refusals_name_the_key(kw, key):
    with pytest.raises(InstantiateFail, match=key):
        model.from_config("attacker", "aia", **kw).I(dataset=_explicit(_ratings()))
    with pytest.raises(InstantiateFail, match="dataset"):
        model.from_config("attacker", "aia").I()


@pytest.mark.parametrize("kw, key", [
    ({"surrogate_model": "ItemAE"}, "surrogate_model"),
    ({"weight_neg_s": 0.5}, "weight_neg_s"),
    ({"optim_g": "SGD"}, "optim_g"),
    ({"hidden_dim_s": 65}, "hidden_dim_s"),
    ({"batch_size_s": 257}, "batch_size_s"),
    ({"unroll_steps_s": 0}, "unroll_steps_s"),
    ({"filler_num": -1}, "filler_num"),
    ({"attack_num": 0}, "attack_num"),
])
@pytest.mark.parametrize("name, cls", [("aia", "AIA"), ("aushplus", "AushPlus")])
def test_shared_refusals_name_the_key_and_the_class(name, cls, kw, key):
    """The refusals AushPlus takes from AIA: raised before any device is asked for, naming the setting and the class built."""
    with pytest.raises(InstantiateFail) as err:
        model.from_config("attacker", name, **kw).I(dataset=_explicit(_ratings()))
    assert key in str(err.value) and f"{cls}:" in str(err.value)


@pytest.mark.parametrize("filler_num", [0, 4, 6])
def test_template_draw_matches_dense_restatement(filler_num):
    mat = _ratings()
    ds = _explicit(mat)
    ptr, idx, val = ds.rating_csr()
    np.random.seed(123)
    users, cols = aia_mod.draw_templates(ptr, idx, val, 9, filler_num)
    after = np.random.random()
    # build_network on the dense train_array, as the reference runs it
    np.random.seed(123)
    sampled = np.random.choice(np.where(np.sum(mat > 0, 1) >= filler_num)[0], 9)
    templates = mat[sampled]
    kept = []
    for template in templates:
        fillers = np.where(template)[0]
        np.random.shuffle(fillers)
        kept.append(fillers[:filler_num])
    assert np.array_equal(users, sampled)
    assert np.array_equal(cols, np.asarray(kept).reshape(9, filler_num))
    assert np.random.random() == after      # the same number of draws
    if filler_num > 3:
        assert 0 not in users.tolist()


def _game_partial():
    """The game data after the reference's partial_sample(0.2) (the rows stored with aush_game_partial)."""
    import os

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aush_game_partial.npz"))
    full = dataset.from_config("explicit", "game", device="cpu", train_dict=g["train_kvr"], valid_dict=g["valid_kvr"],
                               test_dict=g["test_kvr"])
    np.random.seed(int(g["seed"]))
    return full.partial_sample(user_ratio=float(g["user_ratio"]))


@pytest.mark.parametrize("case", ["game_e3", "game_default"])
def test_template_draw_matches_reference_recording(case):
    import os

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"aia_{case}.npz"))
    ptr, idx, val = _game_partial().rating_csr()
    assert [len(idx), idx.astype(np.float64).sum(), val.astype(np.float64).sum()] == g["csr_fp"].tolist()
    F = int(g["cfg_filler_num"]) if "cfg_filler_num" in g else 36
    np.random.seed(int(g["seed"]))
    users, cols = aia_mod.draw_templates(ptr, idx, val, len(g["template_users"]), F)
    assert np.array_equal(users, g["template_users"])
    assert np.array_equal(cols, g["template_cols_drawn"])
    # the generator's positions: the reference's mask nonzeros, row-major with ascending columns
    assert np.array_equal(np.sort(cols, axis=1).reshape(-1), g["pos_cols"])


def test_target_rated_by_every_user_is_refused():
    mat = _ratings()
    mat[:, 2] = 3
    u, i = np.nonzero(mat)
    ptr = np.zeros(mat.shape[0] + 1, dtype=np.int64)
    ptr[1:] = np.cumsum((mat != 0).sum(1))
    users, pptr, _, _, pidx = aia_mod.target_pairs(ptr, i, mat[u, i], mat.shape[0], (1,))
    assert users == np.where(mat[:, 1] == 0)[0].tolist() and pptr == [0, len(users)]
    assert (pidx[0] >= 0).sum() == len(users)
    with pytest.raises(ValueError, match="every real user has rated target 2"):
        aia_mod.target_pairs(ptr, i, mat[u, i], mat.shape[0], (1, 2))


# ---------------------------------------------------------------- the fp64 restatement of the kernels (tests/_aia_restate.py)
# It is the reference of tests/test_aia_kernels_gpu.py, so it is checked here first: against torch autograd in float64, that each
# bound stays under the cap of 2^-10 of its tensor's largest entry, and that each bound rejects a deliberately wrong restatement.
from . import _aia_restate as A  # noqa: E402

# Agreement of two float64 evaluations of the same formula in different orders, relative to the tensor's largest entry: the AUSH
# restatement's 1e-12.  The reverse pass divides by D^2 sqrt(v') and sums O(100) terms of mixed sign per row, so it gets 1e-11.
FP64_RTOL, FP64_RTOL_REV = 1e-12, 1e-11
ADAM_CONST_RTOL = 1e-4


def _close(got, ref, rtol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.abs(got - ref).max() <= rtol * max(np.abs(ref).max(), 1e-300))


def _dense(c, fake=None):
    """X [R, I] as a torch float64 tensor; the fake entries (k >= nnz_real) taken from `fake` when given."""
    rows = torch.as_tensor(np.repeat(np.arange(c.R), np.diff(c.rowptr)))
    vals = torch.as_tensor(c.x.astype(np.float64))
    if fake is not None:
        vals = torch.cat([vals[: c.nnz_real], fake])
    return torch.zeros(c.R, c.I, dtype=torch.float64).index_put((rows, torch.as_tensor(c.col.astype(np.int64))), vals)


def _torch_step(case, th, m, v, X, g_leaf=None):
    """One step in torch float64 with the device's fp32 constants: returns (theta', m', v', g)."""
    c = case.c
    w1, b2, w2, step, bc2s, eps = A.adam_consts(c.lr, c.b1, c.b2, c.eps, case.adam_t)
    b = torch.as_tensor(case.rows)
    Xb = X[b]
    loss = ((Xb > 0).to(torch.float64) * A.f32(c.w) * (Xb - th[b] @ th[c.R:].t()) ** 2).sum()
    (g,) = torch.autograd.grad(loss, th, create_graph=True)
    g = g + A.f32(c.wd) * th
    gg = g if g_leaf is None else g_leaf
    m1 = m + w1 * (gg - m)
    v1 = v * b2 + w2 * gg * gg
    return th - step * (m1 / (torch.sqrt(v1) / bc2s + eps)), m1, v1, g


def _leaves(case):
    return [torch.tensor(a.astype(np.float64), requires_grad=True) for a in (case.theta, case.m, case.v)]


@pytest.mark.parametrize("name", list(A.WMF_CASES))
def test_restated_step_against_autograd(name):
    case = A.wmf_case(name)
    c = case.c
    assert np.array_equal(case.rows, A.batch_rows(c, case.perm, case.j))
    (p1, m1, v1), _ = A.step_ref(c, case.theta, case.m, case.v, case.perm, case.j, case.adam_t)
    th, m, v = _leaves(case)
    tp, tm, tv, _ = _torch_step(case, th, m, v, _dense(c))
    for got, ref in ((p1, tp), (m1, tm), (v1, tv)):
        assert _close(got, ref.detach().numpy(), FP64_RTOL)
    assert not p1[:, c.d:].any() and not m1[:, c.d:].any() and not v1[:, c.d:].any()
    if name == "d16_b40":
        # torch.optim.Adam itself, state preset: it differs from the device by the fp32 rounding of lr, the betas, eps and the two
        # step coefficients.  The largest is 1 - beta2: fp32(0.999) is off by up to 2^-25, which is 2^-25 / 0.001 = 3e-5 of 1 - beta2
        # and so at most that of v' and of the update (ADAM_CONST_RTOL = 1e-4 of the largest update)
        p = torch.nn.Parameter(torch.tensor(case.theta.astype(np.float64)))
        opt = torch.optim.Adam([p], lr=c.lr, betas=(c.b1, c.b2), eps=c.eps, weight_decay=c.wd)
        opt.state[p] = {"step": torch.tensor(float(case.adam_t - 1)), "exp_avg": torch.tensor(case.m.astype(np.float64)),
                        "exp_avg_sq": torch.tensor(case.v.astype(np.float64))}
        Xb = _dense(c)[torch.as_tensor(case.rows)]
        ((Xb > 0).to(torch.float64) * c.w * (Xb - p[torch.as_tensor(case.rows)] @ p[c.R:].t()) ** 2).sum().backward()
        opt.step()
        assert np.abs(p.detach().numpy() - p1).max() <= ADAM_CONST_RTOL * np.abs(p1 - case.theta).max()


@pytest.mark.parametrize("name", list(A.WMF_CASES))
def test_restated_reverse_against_autograd(name):
    case = A.wmf_case(name)
    c = case.c
    (_, m1_64, v1_64), _ = A.step_ref(c, case.theta, case.m, case.v, case.perm, case.j, case.adam_t)
    m1, v1 = m1_64.astype(np.float32), v1_64.astype(np.float32)             # slot k + 1 as the device holds it
    out = A.reverse_ref(c, case.theta, m1, v1, *case.adj, case.perm, case.j, case.adam_t)
    th, m, v = _leaves(case)
    fake = torch.tensor(c.x[c.nnz_real:].astype(np.float64), requires_grad=True)
    X = _dense(c, fake)
    _, _, _, g = _torch_step(case, th, m, v, X)
    # theta', m', v' as functions of (theta, m, v, g) at the m', v' the restatement was given: reverse_ref takes slot k + 1 as data
    w1, b2, w2, step, bc2s, eps = A.adam_consts(c.lr, c.b1, c.b2, c.eps, case.adam_t)
    a_th, a_m, a_v = (torch.tensor(a.astype(np.float64)) for a in case.adj)
    live = torch.as_tensor(v1 > 0)
    mo, vo = torch.tensor(m1.astype(np.float64), requires_grad=True), torch.tensor(np.where(v1 > 0, v1, 1.0).astype(np.float64), requires_grad=True)
    th1 = -step * (mo / (torch.sqrt(vo) / bc2s + eps))
    d_mo, d_vo = torch.autograd.grad((a_th * th1).sum(), (mo, vo))
    mh = a_m + torch.where(live, d_mo, -step * a_th / eps)
    vh = a_v + torch.where(live, d_vo, torch.zeros_like(d_vo))               # the header's rule at v' == 0
    gbar = w1 * mh + 2 * w2 * g.detach() * vh
    assert _close(out["gbar"][0], gbar.numpy(), FP64_RTOL_REV)
    assert _close(out["adj_m"][0], (A.f32(c.b1) * mh).numpy(), FP64_RTOL_REV)
    assert _close(out["adj_v"][0], (b2 * vh).numpy(), FP64_RTOL_REV)
    d_th, d_x = torch.autograd.grad((gbar * g).sum(), (th, fake), retain_graph=True)
    assert _close(out["adj_th"][0], (a_th + d_th).numpy(), FP64_RTOL_REV)
    assert _close(out["xbar"][0], d_x.numpy(), FP64_RTOL_REV)
    if "vzero_row" not in case.facts:
        # and end to end: autograd through the whole step from (theta, m, v), where no v' is 0 (the pad columns' v set to 1: their
        # incoming adjoints are 0, so they add nothing, but sqrt'(0) would make that 0 * inf).  reverse_ref is given the step's own
        # unrounded m', v' here, so both sides differentiate the same float64 function
        out = A.reverse_ref(c, case.theta, m1_64, v1_64, *case.adj, case.perm, case.j, case.adam_t)
        keep = torch.zeros_like(th)
        keep[:, : c.d] = 1
        v = (v.detach() + (1 - keep)).requires_grad_()
        tp, tm, tv, _ = _torch_step(case, th, m, v, X)
        tot = (a_th * tp).sum() + (a_m * tm).sum() + (a_v * tv).sum()
        e_th, e_m, e_v, e_x = torch.autograd.grad(tot, (th, m, v, fake))
        for key, ref in (("adj_th", e_th), ("adj_m", e_m), ("adj_v", e_v), ("xbar", e_x)):
            ref = (ref * keep).numpy() if key != "xbar" else ref.numpy()
            assert _close(out[key][0], ref, FP64_RTOL_REV), key


@pytest.mark.parametrize("name", list(A.LOSS_CASES))
def test_restated_attack_loss_against_log_softmax(name):
    case = A.loss_case(name)
    c = case.c
    (loss, _), (adj, _) = A.attack_loss_ref(*A.loss_args(case), wide=case.wide)
    th = torch.tensor(case.theta.astype(np.float64), requires_grad=True)
    G = Gs = 0.0
    for s, t in enumerate(case.tgt):
        users = torch.as_tensor(case.pair_user[case.pair_ptr[s]:case.pair_ptr[s + 1]].astype(np.int64))
        su = th[users] @ th[c.R:].t()
        # the mask from the restatement's own elementwise scores: a BLAS product need not give equal bits for equal rows
        sc = np.stack([sum(case.theta[u, d].astype(np.float64) * case.theta[c.R:, d].astype(np.float64) for d in range(c.dpad)) for u in users.numpy()])
        mask = torch.as_tensor(sc >= sc[:, t:t + 1])
        nll = -torch.log_softmax(su * mask, -1)[:, t]
        G = G + (nll / 1.1).mean()
        Gs = Gs + float(case.tscale[s]) * nll.sum()      # the gradient's scale is the caller's fp32 tscale = 1 / (11 n), taken as it is
    G = G / 10
    (ref,) = torch.autograd.grad(Gs, th)
    assert abs(loss - float(G.detach())) <= FP64_RTOL * abs(float(G.detach()))
    assert abs(float(Gs.detach()) - float(G.detach())) <= 2.0 ** -23 * abs(float(G.detach()))      # the two scales: fp32(1 / (11 n))
    assert _close(adj, ref.numpy(), FP64_RTOL)
    assert not adj[c.n_real:c.R].any()
    if name == "ties":
        assert len(case.dup) == 2 and all(np.array_equal(case.theta[c.R + i], case.theta[c.R + case.tgt[0]]) for i in case.dup)
    if name == "overflow":
        assert (case.theta[: c.n_real].astype(np.float64) @ case.theta[c.R:].astype(np.float64).T).max() > 90
    if len(case.tgt) > 1:
        assert (case.pidx[:2, 0] >= 0).all() and (case.pidx[:, 1] < 0).all()
    assert len(case.pair_user) % 4 and all(n % 4 for n in np.diff(case.pair_ptr))


def test_restated_project_and_g_step():
    gen = np.array([0.5, 1.5, 2.5, -0.5, -0.0, 0.0, 4.5, 5.5, 7.0, -3.0, 2.4999, 3.5], dtype=np.float32)
    assert np.array_equal(A.project_ref(gen), np.array([0, 2, 2, 0, 0, 0, 4, 5, 5, 0, 2, 4], dtype=np.float32))
    p, m, v, (g, _, _) = A.g_case(50, 3)
    (p1, m1, v1), _ = A.g_step_ref(p, m, v, g, 1e-2, 0.9, 0.999, 1e-8, 3)
    pt = torch.nn.Parameter(torch.tensor(p.astype(np.float64)))
    opt = torch.optim.Adam([pt], lr=1e-2)
    opt.state[pt] = {"step": torch.tensor(2.0), "exp_avg": torch.tensor(m.astype(np.float64)), "exp_avg_sq": torch.tensor(v.astype(np.float64))}
    pt.grad = torch.tensor(g.astype(np.float64))
    opt.step()
    assert np.abs(pt.detach().numpy() - p1).max() <= ADAM_CONST_RTOL * np.abs(p1 - p).max()        # the fp32 constants, as above


# ---------------------------------------------------------------- every bound a GPU test uses is under the cap
def _wmf_refs(case):
    c = case.c
    fwd, fwd_e = A.step_ref(c, case.theta, case.m, case.v, case.perm, case.j, case.adam_t)
    m1, v1 = fwd[1].astype(np.float32), fwd[2].astype(np.float32)
    return fwd, fwd_e, A.reverse_ref(c, case.theta, m1, v1, *case.adj, case.perm, case.j, case.adam_t)


@pytest.mark.parametrize("name", list(A.WMF_CASES))
def test_step_and_reverse_bounds_are_under_the_cap(name):
    case = A.wmf_case(name)
    fwd, fwd_e, rev = _wmf_refs(case)
    for ref, bound in zip(fwd, fwd_e):
        assert A.capped(ref, bound)
    for key, (ref, bound) in rev.items():            # whole tensors, the v' == 0 row included
        assert np.abs(ref).max() > 0 and A.capped(ref, bound), key


@pytest.mark.parametrize("name", list(A.LOSS_CASES))
def test_attack_loss_bounds_are_under_the_cap(name):
    case = A.loss_case(name)
    c = case.c
    (loss, le), (adj, ae) = A.attack_loss_ref(*A.loss_args(case), wide=case.wide)
    assert A.capped(np.array([loss]), np.array([le]))
    assert A.capped(adj[: c.n_real], ae[: c.n_real]) and A.capped(adj[c.R:], ae[c.R:])


@pytest.mark.parametrize("n, t", [(1, 1), (256, 1), (257, 1000)])
def test_g_step_bounds_are_under_the_cap(n, t):
    p, m, v, grads = A.g_case(n, t)
    for k, g in enumerate(grads):
        ref, err = A.g_step_ref(p, m, v, g, 1e-2, 0.9, 0.999, 1e-8, t + k)
        for r, e in zip(ref, err):
            assert A.capped(r, e)
        p, m, v = (a.astype(np.float32) for a in ref)


# ---------------------------------------------------------------- each bound rejects a wrong restatement
@pytest.mark.parametrize("flaw, name, keys", [
    ("no_wd_gbar", "d20_b33", ("adj_th",)),
    ("no_wd_gbar", "betas", ("adj_th",)),
    ("xbar_no_w", "d1_b16", ("xbar",)),
    ("xbar_no_w", "d20_b33", ("xbar",)),
    ("first_block_only", "d16_b40", ("theta", "m", "v", "gbar", "adj_th")),
    ("first_block_only", "d20_b33", ("theta", "m", "v", "gbar", "adj_th")),
    ("factor2", "d32_b32", ("theta", "m", "v", "gbar", "adj_th", "xbar")),
])
def test_bounds_reject_wrong_steps(flaw, name, keys):
    case = A.wmf_case(name)
    c = case.c
    fwd, fwd_e, rev = _wmf_refs(case)
    bad_fwd, _ = A.step_ref(c, case.theta, case.m, case.v, case.perm, case.j, case.adam_t, flaw=flaw)
    bad_rev = A.reverse_ref(c, case.theta, fwd[1].astype(np.float32), fwd[2].astype(np.float32), *case.adj, case.perm, case.j, case.adam_t,
                            flaw=flaw)
    for key in keys:
        if key in ("theta", "m", "v"):
            k = ("theta", "m", "v").index(key)
            assert not A.within(bad_fwd[k], fwd[k], fwd_e[k]), key
        else:
            assert not A.within(bad_rev[key][0], *rev[key]), key


def test_bounds_reject_a_strict_tie_and_a_factor():
    case = A.loss_case("ties")
    c = case.c
    (loss, le), (adj, ae) = A.attack_loss_ref(*A.loss_args(case))
    (bad, _), (bad_adj, _) = A.attack_loss_ref(*A.loss_args(case), flaw="strict_tie")
    assert abs(bad - loss) > le and not A.within(bad_adj, adj, ae)
    assert abs(2 * loss - loss) > le and not A.within(2 * adj, adj, ae)
    # the weight of a stored 0 must be 0: a rating of 0 that weighed w_pos would move its row and its item
    case = A.wmf_case("d16_b40")
    fwd, fwd_e, _ = _wmf_refs(case)
    x = case.c.x.copy()
    zr = case.facts["zero_rating"]
    assert x[case.c.rowptr[zr + 1] - 1] == 0
    case.c.x = np.where(x == 0, np.float32(1e-30), x)              # positive, so weighed, and numerically still 0
    bad, _ = A.step_ref(case.c, case.theta, case.m, case.v, case.perm, case.j, case.adam_t)
    assert not A.within(bad[0], fwd[0], fwd_e[0])


def test_restatement_refuses_a_near_tie():
    case = A.loss_case("i37_u5")
    c = case.c
    t, u = int(case.pair_tgt[0]), int(case.pair_user[0])
    i = (t + 1) % c.I
    case.theta[c.R + i] = case.theta[c.R + t]
    d = int(np.argmax(np.abs(case.theta[u])))
    case.theta[c.R + i, d] = np.nextafter(case.theta[c.R + i, d], np.float32(9))      # one ulp off an exact tie
    with pytest.raises(AssertionError, match="within rounding"):
        A.attack_loss_ref(*A.loss_args(case))
