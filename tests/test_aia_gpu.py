"""GPU tests of the AIA attacker (csrc/aia.hip + recad_amd/attack/aia.py): the unrolled epochs, attack loss and reverse pass
against a float64 torch autograd restatement (create_graph through every Adam step) from the device's own draws and state,
the checkpointed reverse against the full-history one, run-to-run bit-identity, filler_num 0 and both workflows.

Tolerances.  The restatement starts from the device's state at entry to the unrolled epochs, so only those epochs, the loss
and the reverse differ, and only by fp32 rounding: the loss within 1e-5 relative (a mean of O(users) log-softmax terms);
theta after the unrolled epochs within 1e-4 absolute (O(10) Adam steps of lr 1e-2 per row); the hypergradient within 1e-3
relative in norm, with the sign equal wherever |X-bar| is above 1e-3 of its max (G's first Adam step moves each entry by
lr_g sign(X-bar), so the sign is what acts)."""
import os

import numpy as np
import pytest
import torch

from recad_amd import dataset, model, synth, workflow
from recad_amd.defense.pca_select_users import flag_count

pytestmark = pytest.mark.gpu
LOSS_RTOL = 1e-5
THETA_ATOL = 1e-4
XBAR_RTOL = 1e-3


def _synth(dev, n_users=150, n_items=90, seed=3):
    rng = np.random.default_rng(seed)
    mat = np.where(rng.random((n_users, n_items)) < 0.2, rng.integers(1, 6, (n_users, n_items)), 0).astype(np.float32)
    mat[:, 0] = np.where(rng.random(n_users) < 0.3, 5, 0)         # target 0: rated by some users only
    u, i = np.nonzero(mat)
    kvr = np.stack([u, i, mat[u, i].astype(np.int64)], 1)
    return dataset.from_config("explicit", "synth", device=dev, train_dict=kvr), mat


def _aia(ds, dev, np_seed=5, torch_seed=11, **kw):
    cfg = dict(attack_num=10, filler_num=6, epoch_s=3, unroll_steps_s=1, batch_size_s=16, device=dev)
    cfg.update(kw)
    np.random.seed(np_seed)
    torch.manual_seed(torch_seed)
    return model.from_config("attacker", "aia", **cfg).I(dataset=ds)


def _restate(att, mat, targets):
    """float64 restatement of the unrolled epochs + attack loss (aia.py:463-489, 88-114) from the device's entry state.
    Returns (loss, xbar [A, F], P, Q after the unrolled epochs)."""
    e = att.entry_state()
    U, I, A, F = att.n_users, att.n_items, att.attack_num, att.filler_num
    dd = torch.float64
    fake = torch.tensor(att._x[att.nnz_real:].cpu().numpy().astype(np.float64).reshape(A, F), requires_grad=True)
    X = torch.zeros(U + A, I, dtype=dd)
    X[:U] = torch.as_tensor(mat[:U, :I], dtype=dd)
    rows = torch.arange(A).repeat_interleave(F)
    X = X.index_put((rows + U, torch.as_tensor(att.template_cols.reshape(-1))), fake.reshape(-1))
    P = torch.tensor(e["P"], dtype=dd, requires_grad=True)
    Q = torch.tensor(e["Q"], dtype=dd, requires_grad=True)
    mP, mQ = torch.tensor(e["mP"], dtype=dd), torch.tensor(e["mQ"], dtype=dd)
    vP, vQ = torch.tensor(e["vP"], dtype=dd), torch.tensor(e["vQ"], dtype=dd)
    t = e["adam_t"]
    b1, b2, eps, lr, wd, w = 0.9, 0.999, 1e-8, att.lr_s, att.wd_s, att.w_pos
    for perm in e["perms"]:
        for s in range(0, len(perm), att.batch):
            b = torch.as_tensor(perm[s:s + att.batch].astype(np.int64))
            Xb = X[b]
            loss = ((Xb > 0).to(dd) * w * (Xb - P[b] @ Q.t()) ** 2).sum()
            gP, gQ = torch.autograd.grad(loss, (P, Q), create_graph=True)
            t += 1
            bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
            new = []
            for p, g, m, v in ((P, gP + wd * P, mP, vP), (Q, gQ + wd * Q, mQ, vQ)):
                m = b1 * m + (1 - b1) * g
                v = b2 * v + (1 - b2) * g * g
                new.append((p - lr / bc1 * m / (torch.sqrt(v) / np.sqrt(bc2) + eps), m, v))
            (P, mP, vP), (Q, mQ, vQ) = new
    s = P[:U] @ Q.t()
    G = 0.0
    for tg in targets:
        users = np.where(mat[:, tg] == 0)[0]
        su = s[users]
        z = su * (su >= su[:, tg:tg + 1]).to(dd)
        G = G + (-torch.log_softmax(z, -1)[:, tg] / 1.1).mean()
    G = G / 10
    (xbar,) = torch.autograd.grad(G, fake)
    return float(G.detach()), xbar.numpy(), P.detach().numpy(), Q.detach().numpy()


def _check_xbar(got, ref):
    assert np.linalg.norm(got - ref) <= XBAR_RTOL * np.linalg.norm(ref), (np.linalg.norm(got - ref), np.linalg.norm(ref))
    big = np.abs(ref) > 1e-3 * np.abs(ref).max()
    assert np.array_equal(np.sign(got[big]), np.sign(ref[big]))


@pytest.mark.parametrize("unroll, batch", [(1, 16), (2, 16), (1, 7), (2, 7)])
def test_unrolled_reverse_against_fp64(gpu_device, unroll, batch):
    ds, mat = _synth(gpu_device)
    targets = [0, 5]
    att = _aia(ds, gpu_device, unroll_steps_s=unroll, batch_size_s=batch)
    if batch == 7:
        assert att.R % 7 != 0          # a short last batch
    x0 = att._x[att.nnz_real:].clone()
    gen0 = att.generator_values().copy()
    (loss,) = att.train_step(target_id_list=targets)
    # the restatement runs on the projection the step used (before its G update)
    x_after = att._x[att.nnz_real:].clone()
    att._x[att.nnz_real:] = x0
    ref_loss, ref_xbar, P, Q = _restate(att, mat, targets)
    att._x[att.nnz_real:] = x_after
    assert abs(loss - ref_loss) <= LOSS_RTOL * abs(ref_loss), (loss, ref_loss)
    got = att.last_hypergradient()
    _check_xbar(got, ref_xbar)
    # G's first Adam step: m-hat = g, v-hat = g^2, so each entry moves by -lr_g g / (|g| + eps)
    moved = att.generator_values().astype(np.float64) - gen0
    assert np.allclose(moved, -att.lr_g * got / (np.abs(got) + 1e-8), rtol=0, atol=2e-6)
    # the surrogate after the unrolled epochs, through the low-level entry from the same state
    e = att.last_entry
    dp = torch.as_tensor(e["perms"]).to(gpu_device)
    inv = torch.as_tensor(np.argsort(e["perms"], axis=1).astype(np.int32)).to(gpu_device)
    att._x[att.nnz_real:] = x0
    l2, xb2, final = att.unrolled(e["state"], e["adam_t"], dp, inv, targets)
    att._x[att.nnz_real:] = x_after
    assert float(l2.cpu()[0]) == loss
    assert torch.equal(xb2.cpu(), att.last_xbar.cpu())
    Pd, Qd = att.state_to_numpy(final)
    assert np.abs(Pd - P).max() <= THETA_ATOL and np.abs(Qd - Q).max() <= THETA_ATOL


def test_padded_dim_against_fp64(gpu_device):
    ds, mat = _synth(gpu_device, seed=4)
    att = _aia(ds, gpu_device, hidden_dim_s=20, epoch_s=2)
    assert att.dpad == 32
    x0 = att._x[att.nnz_real:].clone()
    (loss,) = att.train_step(target_id_list=[0])
    att._x[att.nnz_real:] = x0
    ref_loss, ref_xbar, _, _ = _restate(att, mat, [0])
    assert abs(loss - ref_loss) <= LOSS_RTOL * abs(ref_loss)
    _check_xbar(att.last_hypergradient(), ref_xbar)


@pytest.mark.parametrize("batch", [16, 7])
def test_checkpointed_reverse_is_bit_identical(gpu_device, batch):
    ds, _ = _synth(gpu_device)
    runs = []
    for cap in (None, 1):      # full history, then a cap that forces checkpoints every ceil(sqrt(K)) steps
        kw = {} if cap is None else {"history_bytes": cap}
        att = _aia(ds, gpu_device, unroll_steps_s=2, batch_size_s=batch, **kw)
        if batch == 7:         # 23 steps per epoch, K = 46, segments of 7: segments cross the epoch boundary
            nb = att._nsteps()
            assert any(a // nb != (b - 1) // nb for a, b in [(a, min(a + 7, 2 * nb)) for a in range(0, 2 * nb, 7)])
        torch.manual_seed(17)
        np.random.seed(9)
        (loss,) = att.train_step(target_id_list=[0, 5])
        runs.append((loss, att.last_hypergradient(), att.generator_values(), att.last_history))
    assert runs[0][3]["full"] and not runs[1][3]["full"] and runs[1][3]["segment"] < runs[1][3]["steps"]
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])


def test_run_to_run_bit_identity(gpu_device):
    ds, _ = _synth(gpu_device)
    out = []
    for _ in range(2):
        att = _aia(ds, gpu_device)
        losses = [att.train_step(target_id_list=[0])[0] for _ in range(2)]
        out.append((losses, att.last_hypergradient(), att.generate_fake(target_id_list=[0])))
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


def test_filler_num_zero(gpu_device):
    ds, _ = _synth(gpu_device)
    att = _aia(ds, gpu_device, filler_num=0)
    (loss,) = att.train_step(target_id_list=[0])
    assert np.isfinite(loss)
    assert att.last_hypergradient().shape == (10, 0) and att.generator_values().shape == (10, 0)
    fake = att.generate_fake(target_id_list=[0])
    assert fake.shape == (10, att.n_items) and fake.dtype == np.float32
    assert np.array_equal(np.nonzero(fake)[1], np.zeros(10))


def test_generate_fake_and_refused_target(gpu_device):
    ds, mat = _synth(gpu_device)
    att = _aia(ds, gpu_device)
    att.train_step(target_id_list=[0, 5])
    fake = att.generate_fake(target_id_list=[0, 5])
    assert fake.shape == (10, att.n_items)
    x = np.clip(np.rint(att.generator_values()), 0, 5)
    expect = np.zeros_like(fake)
    np.put_along_axis(expect, att.template_cols, x, axis=1)
    expect[:5, 0] = 5
    expect[5:, 5] = 5
    assert np.array_equal(fake, expect)
    mat2 = mat.copy()
    mat2[:, 1] = 3
    u, i = np.nonzero(mat2)
    ds2 = dataset.from_config("explicit", "all", device=gpu_device, train_dict=np.stack([u, i, mat2[u, i].astype(np.int64)], 1))
    with pytest.raises(ValueError, match="every real user"):
        _aia(ds2, gpu_device).train_step(target_id_list=[1])


# ---------------------------------------------------------------- workflows
def _ml1m_data(dev):
    d = synth.make("ml1m")
    victim = dataset.from_config("implicit", "ml1m", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], device=dev,
                                 graph_source="train", seed=5)
    r = synth.with_ratings(d)
    explicit = dataset.from_config("explicit", "ml1m", train_csr=r["train"], valid_csr=r["valid"], test_csr=r["test"], device=dev)
    np.random.seed(7)
    return victim, explicit, explicit.partial_sample(user_ratio=0.2)


def test_no_defense_workflow_with_aia(gpu_device):
    victim_data, _, attack_data = _ml1m_data(gpu_device)
    wf = workflow.from_config("no defense", victim_data=victim_data, attack_data=attack_data,
                              victim=model.from_config("victim", "lightgcn", latent_dim_rec=32, lightGCN_n_layers=2),
                              attacker=model.from_config("attacker", "aia", device=gpu_device, epoch_s=5),
                              rec_epoch=1, attack_epoch=2, target_id_list=[0], device=gpu_device)
    res = wf.execute()
    assert res["n_eval_users"] > 0
    assert all(np.isfinite(v) for v in res.values())
    assert wf.fake_dataset.n_users > victim_data.n_users


def test_defense_workflow_with_aia(gpu_device):
    victim_data, explicit, attack_data = _ml1m_data(gpu_device)
    wf = workflow.from_config("defense", victim_data=victim_data, attack_data=attack_data, defense_data=explicit,
                              victim=model.from_config("victim", "lightgcn", latent_dim_rec=32, lightGCN_n_layers=2),
                              attacker=model.from_config("attacker", "aia", device=gpu_device),
                              defender=model.from_config("defender", "PCASelectUsers", device=gpu_device),
                              rec_epoch=1, attack_epoch=1, target_id_list=[0], device=gpu_device)
    res = wf.execute()
    assert wf.defender.user_num == wf.fake_dataset.n_users
    assert res["n_flagged"] == flag_count(50, wf.fake_dataset.n_users) == 50


# ---------------------------------------------------------------- replay of the reference's own runs (make_golden_aia.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(name):
    return np.load(os.path.join(GOLDEN, f"aia_{name}.npz"))


def _game_partial(dev):
    g = np.load(os.path.join(GOLDEN, "aush_game_partial.npz"))
    full = dataset.from_config("explicit", "game", device=dev, train_dict=g["train_kvr"], valid_dict=g["valid_kvr"],
                               test_dict=g["test_kvr"])
    np.random.seed(int(g["seed"]))
    return full.partial_sample(user_ratio=float(g["user_ratio"]))


def _fp(a):
    a = np.asarray(a, dtype=np.float64)
    return np.asarray([a.sum(), (a * a).sum()])


# Tolerances of the whole-train_step replays: the issue's -- G_loss 1e-5 relative, theta at the unrolled entry 1e-4, the
# hypergradient 1e-3 relative in norm with every sign equal above 1e-3 of its max -- except theta for default.  There the
# entry comes after 49 plain epochs (2 107 Adam steps) of fp32 summed in another order than torch's CPU kernels; Adam divides
# by sqrt(v), so entries whose gradient is near 0 take steps of either sign and the reordering differences do not shrink
# with the step count.  Measured on MI355X: theta 8.2e-4 (loss 4.0e-7, hypergradient 3.8e-4, all signs equal), so 2e-3.
# e3 reaches theta 4.4e-6, loss 1.5e-7, hypergradient 1.1e-4.
REPLAY = {"game_e3": {"loss": 1e-5, "theta": 1e-4, "xbar": 1e-3},
          "game_default": {"loss": 1e-5, "theta": 2e-3, "xbar": 1e-3}}


@pytest.mark.parametrize("case", ["game_e3", "game_default"])
def test_replay_of_reference_train_steps(gpu_device, case):
    g = _golden(case)
    tol = REPLAY[case]
    ds = _game_partial(gpu_device)
    cfg = {k[4:]: v.item() for k, v in g.items() if k.startswith("cfg_")}
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    att = model.from_config("attacker", "aia", device=gpu_device, **cfg).I(dataset=ds)
    assert np.array_equal(att.template_users, g["template_users"])
    assert np.array_equal(att.template_cols.reshape(-1), g["pos_cols"])
    targets = g["targets"].tolist()
    for s in range(int(g["steps"])):
        (loss,) = att.train_step(target_id_list=targets)
        assert abs(loss - g["g_loss"][s]) <= tol["loss"] * abs(g["g_loss"][s]), (case, s, loss, g["g_loss"][s])
        e = att.entry_state()
        assert e["adam_t"] == g["entry_step"][s]
        P, Q = e["P"], e["Q"]
        assert np.abs(P[g["sample_P"]] - g["entry_P_rows"][s]).max() <= tol["theta"], np.abs(P[g["sample_P"]] - g["entry_P_rows"][s]).max()
        assert np.abs(Q[g["sample_Q"]] - g["entry_Q_rows"][s]).max() <= tol["theta"]
        assert np.abs(Q[targets[0]] - g["entry_Q_target"][s]).max() <= tol["theta"]
        got_fp = np.concatenate([_fp(e[k]) for k in ("P", "Q", "mP", "mQ", "vP", "vQ")])
        assert np.allclose(got_fp, g["entry_fp"][s], rtol=10 * tol["theta"], atol=0), (got_fp, g["entry_fp"][s])
        xb = att.last_hypergradient().reshape(-1)
        ref = g["xbar"][s]
        assert np.linalg.norm(xb - ref) <= tol["xbar"] * np.linalg.norm(ref), (case, s, np.linalg.norm(xb - ref) / np.linalg.norm(ref))
        big = np.abs(ref) > 1e-3 * np.abs(ref).max()
        assert np.array_equal(np.sign(xb[big]), np.sign(ref[big]))
    fake = att.generate_fake(target_id_list=targets)
    fr, fc = np.nonzero(fake)
    assert np.array_equal(fr, g["fake_rows"]) and np.array_equal(fc, g["fake_cols"])
    assert np.array_equal(fake[fr, fc], g["fake_vals"])


class _DenseData:
    def __init__(self, mat):
        self.mat = mat

    def info_describe(self):
        return {"n_users": self.mat.shape[0], "n_items": self.mat.shape[1], "train_mat": self.mat}


def test_reverse_pass_alone_from_reference_state(gpu_device):
    g = _golden("small_state")
    ptr, idx, val = g["small_ptr"], g["small_idx"], g["small_val"]
    mat = np.zeros((len(ptr) - 1, int(g["n_items"])), dtype=np.float32)
    mat[np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), idx] = val
    cfg = {k[4:]: v.item() for k, v in g.items() if k.startswith("cfg_")}
    np.random.seed(int(g["seed"]))
    torch.manual_seed(int(g["seed"]))
    att = model.from_config("attacker", "aia", device=gpu_device, **cfg).I(dataset=_DenseData(mat))
    assert np.array_equal(att.template_users, g["template_users"])
    assert np.allclose(att.generator_values().reshape(-1), g["state_gen"])
    R, I, d, N = att.R, att.n_items, att.dim, att.N
    st = torch.zeros(3, R + I, att.dpad)
    for k, pre in enumerate(("", "m", "v")):
        st[k, :R, :d] = torch.as_tensor(g["state_" + pre + "P"])
        st[k, R:, :d] = torch.as_tensor(g["state_" + pre + "Q"])
    perms = g["state_perms"].astype(np.int32)
    inv = np.argsort(perms, axis=1).astype(np.int32)
    loss, xbar, _ = att.unrolled(st.reshape(-1).to(gpu_device), int(g["entry_step"][0]), torch.as_tensor(perms).to(gpu_device),
                                 torch.as_tensor(inv).to(gpu_device), g["targets"].tolist())
    ref_loss = float(g["g_loss"][0])
    assert abs(float(loss.cpu()[0]) - ref_loss) <= LOSS_RTOL * abs(ref_loss)
    _check_xbar(xbar.cpu().numpy(), g["xbar"][0])
