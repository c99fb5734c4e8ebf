"""GPU tests of the Mult-VAE victim end to end on a 300 x 120 synthetic dataset (H = 64, L = 16): five epochs against the float64
replay of tests/_multvae_restate.py on the same user orders, masks and noise, the reported losses, both scoring paths, the batched
evaluation against the oracle's top-K of the device's own score matrix, a constructed push through the "no defense" workflow, a
"defense" workflow with KnnSelectUsers, held-out quality, the state_dict round trip with the Adam moments, reset(), a foreign
optimizer, and the repeatability of a training run."""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from recad_amd import dataset, model, synth, workflow
from recad_amd.evaluate import eligible_users, full_catalog_topk, heldout_quality, quality_dict
from recad_amd.victim.multvae import init_flat
from tests import _multvae_restate as R
from tests import _rank_restate as RR

pytestmark = pytest.mark.gpu
U, I, H, L = 300, 120, 64, 16
CFG = dict(hidden_dim=H, latent_dim=L, dropout=0.5, anneal_cap=0.2, total_anneal_steps=10, batch_size=128, lr=0.01, seed=7)
TARGET, N_FAKE, N_POP = 85, 15, 5
EPS64 = 2.0 ** -52
ORDER_SEED = 21


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _data():
    ptr, idx = synth.user_item_edges(U, I, 4300, 3)
    train, valid, test = synth.split_edges(ptr, idx, (3600, 350, 350), 3)
    return {"train": train, "valid": valid, "test": test}


def _small(dev):
    d = _data()
    return dataset.from_config("implicit", "small", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], need_graph=False,
                               device=dev, sample="pairwise", graph_source="train", seed=5)


def _lazy(**kw):
    return model.from_config("victim", "multvae", **{**CFG, **kw})


def _victim(ds, dev, **kw):
    return _lazy(**kw).I(dataset=ds).to(dev)


def _train_csr(ds):
    ptr, idx = ds.train_csr_sorted()
    return np.asarray(ptr).astype(np.int64)[:U + 1], np.asarray(idx).astype(np.int64)


def _orders(ds, n):
    """the user orders n train_steps draw after torch.manual_seed(ORDER_SEED)"""
    ptr, _ = _train_csr(ds)
    users = np.nonzero(np.diff(ptr) > 0)[0]
    torch.manual_seed(ORDER_SEED)
    return [users[torch.randperm(len(users)).numpy()] for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _reference(dev, opt="adam", n=5, lr=CFG["lr"]):
    """the float64 replay and the plain fp32 numpy replay of n epochs from the seeded parameters"""
    ds = _small(dev)
    ptr, idx = _train_csr(ds)
    theta0 = init_flat(I, H, L, CFG["seed"]).numpy()
    kw = dict(batch=CFG["batch_size"], seed=CFG["seed"], dropout=CFG["dropout"], cap=CFG["anneal_cap"], total=CFG["total_anneal_steps"], lr=lr, opt=opt)
    orders = _orders(ds, n)
    t64, l64 = R.replay(theta0, ptr, idx, I, H, L, orders, dt=np.float64, **kw)
    t32, l32 = R.replay(theta0, ptr, idx, I, H, L, orders, dt=np.float32, **kw)
    steps = len(l64) // n
    return {"theta0": theta0, "t64": t64, "l64": np.array(l64).reshape(n, steps), "walk_theta": float(np.max(np.abs(t32 - t64))),
            "walk_loss": np.abs(np.array(l32) - np.array(l64)).reshape(n, steps), "steps": steps}


def test_five_epochs_against_float64(gpu_device):
    """Five train_steps against the float64 replay of the same orders, masks and noise.  The device may end 4 x as far from
    float64 as the plain fp32 numpy replay does, plus 2^-23 max|theta|; the reported losses likewise, plus 2^-23 of the loss.
    The allowance is measured against the reference, never against the device.

    Measured on the MI355X: the numpy replay ends 7.681e-07 from float64, the allowance is 3.147e-06, the device ends 1.794e-07 away
    (0.06 of the allowance) and its epoch losses within 4.1e-8 (allowed 1.2e-5 and more)."""
    ref = _reference(gpu_device)
    ds = _small(gpu_device)
    v = _victim(ds, gpu_device)
    assert np.array_equal(_bits(v.theta.data.cpu().numpy()), _bits(ref["theta0"])) and v.steps_done.tolist() == [0]
    torch.manual_seed(ORDER_SEED)
    for ep in range(5):
        (loss,) = v.train_step(progress_bar=None)
        want = float(ref["l64"][ep].mean())
        allowed = 4 * float(ref["walk_loss"][ep].max()) + 2.0 ** -23 * abs(want)
        print(f"epoch {ep}: device {loss:.9f}, float64 {want:.9f}, |difference| {abs(loss - want):.3e}, allowed {allowed:.3e}")
        assert abs(loss - want) <= allowed
        assert v.last_losses["kl"] > 0 and v.last_losses["nll"] <= loss <= v.last_losses["nll"] + CFG["anneal_cap"] * v.last_losses["kl"] * 1.001
    assert v.steps_done.tolist() == [5 * ref["steps"]] and int(v.optimizer.state[v.theta]["step"]) == 5 * ref["steps"]
    theta = v.theta.data.cpu().numpy()
    dev_theta = float(np.max(np.abs(theta - ref["t64"])))
    allowed = 4 * ref["walk_theta"] + 2.0 ** -23 * float(np.abs(ref["t64"]).max())
    print(f"parameters: device {dev_theta:.3e} from float64, walk {ref['walk_theta']:.3e}, allowed {allowed:.3e}, ratio {dev_theta / allowed:.3f}")
    assert np.abs(ref["t64"] - ref["theta0"]).max() > 1e-2 and dev_theta <= allowed


@functools.lru_cache(maxsize=None)
def _fitted(dev):
    ds = _small(dev)
    v = _victim(ds, dev)
    torch.manual_seed(ORDER_SEED)
    for _ in range(5):
        v.train_step()
    return ds, v


def _score_matrix(v, users, dev):
    ids = torch.as_tensor(np.asarray(users, dtype=np.int32), device=dev)
    out = torch.empty(len(users) * I, dtype=torch.float32, device=dev)
    v.score_matrix(ids, out)
    return out.view(len(users), I).cpu().numpy()


def test_forward_equals_score_matrix_and_float64(gpu_device):
    ds, v = _fitted(gpu_device)
    S = _score_matrix(v, np.arange(U), gpu_device)
    rng = np.random.default_rng(3)
    users, items = rng.integers(0, U, size=700), rng.integers(0, I, size=700)
    pairs = v(torch.as_tensor(users, device=gpu_device), torch.as_tensor(items, device=gpu_device)).cpu().numpy()
    assert np.array_equal(_bits(pairs), _bits(S[users, items])) and np.abs(pairs).max() > 0.01
    ptr, idx = _train_csr(ds)
    want = R.scores64(v.theta.data.cpu().numpy(), ptr, idx, I, H, L, np.arange(U))
    assert np.abs(S - want).max() <= 2.0 ** -14 * np.abs(want).max()
    assert v(torch.zeros(0, dtype=torch.long, device=gpu_device), torch.zeros(0, dtype=torch.long, device=gpu_device)).numel() == 0


def _restated_eval(S, users, targets, K):
    ptr, idx = (np.asarray(a).astype(np.int64) for a in _data()["train"])
    rows = [orc.topk_row(S[u], idx[ptr[u]:ptr[u + 1]], K, np.asarray(targets, dtype=np.int32)) for u in users]
    return [np.stack([r[j] for r in rows]) for j in range(4)]


def test_topk_equals_the_oracle_on_the_device_score_matrix(gpu_device):
    ds, v = _fitted(gpu_device)
    ptr, idx = ds.train_csr_sorted()
    targets = np.array([TARGET, 0], dtype=np.int32)
    users = eligible_users(ptr, idx, targets)
    K = 50
    assert 200 < len(users) < U
    res = full_catalog_topk(v, users, ptr, idx, targets, K=K, chunk=128)         # three chunks
    S = _score_matrix(v, np.arange(U), gpu_device)
    top_ids, top_scores, tscore, trank = _restated_eval(S, users, targets, K)
    assert np.array_equal(_bits(res["top_scores"]), _bits(top_scores))
    assert np.array_equal(_bits(res["target_score"]), _bits(tscore)) and np.array_equal(res["target_rank"], trank)
    tie_free = np.array([len(np.unique(row)) == len(row) for row in top_scores])
    assert tie_free.mean() > 0.9 and np.array_equal(res["top_ids"][tie_free], top_ids[tie_free])


def _push_profile(idx):
    popular = np.argsort(-np.bincount(idx, minlength=I), kind="stable")[:N_POP + 1]
    popular = popular[popular != TARGET][:N_POP]
    return np.sort(np.r_[popular, [TARGET]])


class _PushAttack:
    """Test-local attacker: the constructed push, ratings of 5 so that inject_data(filter_num=4) keeps every item."""

    model_name = "push"

    def __init__(self):
        idx = np.asarray(_data()["train"][1])
        self.fake = np.zeros((N_FAKE, I))
        self.fake[:, _push_profile(idx)] = 5

    def I(self, **kw):
        return self

    def to(self, device):
        return self

    def input_describe(self):
        return {"generate_fake": {"target_id_list": (list, [])}}

    def generate_fake(self, target_id_list, **config):
        assert list(target_id_list) == [TARGET]
        return self.fake


def test_push_attack_through_the_workflow(gpu_device):
    """The float64 run of tests/test_multvae_host.py shows a small lift on `tiny` (0.000 -> 0.014 .. 0.034 over seeds and epoch
    counts), too small to assert a direction here: the run completes and its figures are finite.  Measured on the device:
    HR@10 0.000 -> 0.024, HR@20 0.007 -> 0.128, HR@50 0.052 -> 0.436 over the 289 eligible users."""
    ds = _small(gpu_device)
    torch.manual_seed(5)
    wf = workflow.from_config("no defense", victim_data=ds, attack_data=None, victim=_lazy(), attacker=_PushAttack(), rec_epoch=40,
                              attack_epoch=0, device=gpu_device, target_id_list=[TARGET], topks=[5, 10, 20, 50])
    res = wf.execute()
    assert len(wf.losses) == 40 and wf.fake_dataset.n_users == U + N_FAKE
    print(f"PUSH multvae: HR@10 of item {TARGET} over {res['n_eval_users']} users {res['HR@10']:.3f} -> {res['HR@10 after attack']:.3f}")
    assert res["n_eval_users"] == 289
    assert all(np.isfinite(res[k]) and 0 <= res[k] <= 1 for k in ("HR@10", "HR@10 after attack")) and np.all(np.isfinite(np.asarray(wf.losses, dtype=np.float64)))


def test_defense_workflow_with_knn_defender(gpu_device):
    ds = _small(gpu_device)
    defender = model.from_config("defender", "KnnSelectUsers", k=25, attack_num=N_FAKE, device=gpu_device)
    wf = workflow.from_config("defense", victim_data=ds, attack_data=None, victim=_lazy(), attacker=_PushAttack(), defender=defender,
                              rec_epoch=3, attack_epoch=0, device=gpu_device, target_id_list=[TARGET], topks=[10, 20])
    res = wf.execute()
    assert set(res) == {"attacked", "defended", "n_flagged"} and wf.fake_dataset.n_users == U + N_FAKE
    assert wf.defended_victim.num_users == wf.cleaned_dataset.n_users and wf.defended_victim.steps_done.item() > 0
    assert wf.detection["n_fake"] == N_FAKE
    for part in ("attacked", "defended"):
        assert 0 <= res[part]["HR@10"] <= 1 and 0 <= res[part]["HR@10 after attack"] <= 1


def test_heldout_quality_equals_the_restated_lists(gpu_device):
    ds, v = _fitted(gpu_device)
    topks = (10, 20)
    S = _score_matrix(v, np.arange(U), gpu_device)
    for split in ("test", "valid"):
        got = heldout_quality(v, ds, split=split, topks=topks)
        gt_ptr, gt_idx = ds.heldout_csr(split)
        users = np.nonzero(np.diff(gt_ptr))[0].astype(np.int32)
        top = _restated_eval(S, users, [], 20)[0]
        ref = quality_dict(RR.rank_metrics(top, users, gt_ptr, gt_idx, topks, RR.discount_table(20))[3], topks)
        assert got["n_quality_users"] == ref["n_quality_users"] == len(users) > 0
        for name, r in ref.items():
            assert abs(got[name] - r) <= (len(users) + 100) * EPS64 * abs(r), (split, name)
        assert 0 <= got["Recall@10"] <= got["Recall@20"] <= 1
    print(f"QUALITY multvae after 5 epochs: {heldout_quality(v, ds, split='test', topks=topks)}")


def test_state_dict_round_trip_with_the_adam_moments(gpu_device):
    ds, v = _fitted(gpu_device)
    steps = _reference(gpu_device)["steps"]
    state = {k: t.clone() for k, t in v.state_dict().items()}
    opt = copy.deepcopy(v.optimizer.state_dict())
    assert set(state) == {"theta", "steps_done"} and state["steps_done"].tolist() == [5 * steps]
    assert opt["state"][0]["exp_avg"].shape == (R.n_params(I, H, L),) and bool(opt["state"][0]["exp_avg"].any()) and int(opt["state"][0]["step"]) == 5 * steps
    fresh = _lazy().I(dataset=ds)
    fresh.load_state_dict({k: t.cpu() for k, t in state.items()})
    fresh.optimizer.load_state_dict(opt)
    fresh = fresh.to(gpu_device)
    assert fresh.steps_done.tolist() == [5 * steps] and torch.equal(fresh.theta.data, v.theta.data)
    twin = _lazy().I(dataset=ds).to(gpu_device)
    twin.load_state_dict(v.state_dict())
    twin.optimizer.load_state_dict(copy.deepcopy(v.optimizer.state_dict()))
    torch.manual_seed(9)
    a = fresh.train_step()
    torch.manual_seed(9)
    b = twin.train_step()
    assert a == b and torch.equal(fresh.theta.data, twin.theta.data), "a loaded model goes on from where the saved one was"
    assert fresh.steps_done.tolist() == [6 * steps]
    cold = _lazy().I(dataset=ds).to(gpu_device)
    cold.load_state_dict(v.state_dict())
    torch.manual_seed(9)
    cold.train_step()
    assert not torch.equal(cold.theta.data, twin.theta.data), "without the moments the step differs"


def test_reset_gives_an_untrained_model(gpu_device):
    ds, v = _fitted(gpu_device)
    lazy = v.reset()
    assert not lazy._is_instantiate and lazy._init_config["dropout"] == CFG["dropout"]
    again = lazy.I(dataset=ds).to(gpu_device)
    assert again.steps_done.tolist() == [0]
    assert np.array_equal(_bits(again.theta.data.cpu().numpy()), _bits(_reference(gpu_device)["theta0"]))
    assert v.reset(hidden_dim=33).I(dataset=ds).W1.shape == (I, 33)


def test_a_foreign_optimizer_steps_on_the_restated_gradients(gpu_device):
    """SGD through _unfused_epoch (the library returns each minibatch's flat gradient, torch steps): two epochs against the
    float64 replay with p -= lr g, under the idiom of the five-epoch test."""
    ref = _reference(gpu_device, opt="sgd", n=2, lr=0.05)
    ds = _small(gpu_device)
    v = _victim(ds, gpu_device, optim="SGD", lr=0.05)
    assert not v._fused_adam
    torch.manual_seed(ORDER_SEED)
    for ep in range(2):
        (loss,) = v.train_step()
        assert abs(loss - ref["l64"][ep].mean()) <= 1e-4 * abs(loss)
    theta = v.theta.data.cpu().numpy()
    dev = float(np.max(np.abs(theta - ref["t64"])))
    print(f"SGD parameters: device {dev:.3e} from float64, walk {ref['walk_theta']:.3e}")
    assert np.abs(ref["t64"] - ref["theta0"]).max() > 1e-3 and dev <= 4 * ref["walk_theta"] + 2.0 ** -23 * float(np.abs(ref["t64"]).max())
    assert v.steps_done.tolist() == [2 * ref["steps"]]


def test_two_trainings_from_one_seed_give_the_same_bits(gpu_device):
    out = []
    for _ in range(2):
        ds = _small(gpu_device)
        v = _victim(ds, gpu_device, seed=3)
        torch.manual_seed(4)
        losses = [v.train_step() for _ in range(4)]
        out.append((losses, v.theta.data.cpu().numpy(), dict(v.last_losses)))
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2]
    assert np.array_equal(_bits(out[0][1]), _bits(out[1][1])) and out[0][1].any()


def test_a_user_without_items_never_enters_an_epoch_and_scores_from_the_biases(gpu_device):
    d = _data()
    ptr, idx = (np.asarray(a).copy() for a in d["train"])
    cut = int(ptr[8] - ptr[7])
    idx = np.r_[idx[:ptr[7]], idx[ptr[8]:]]
    ptr[8:] -= cut
    ds = dataset.from_config("implicit", "small", train_csr=(ptr, idx), valid_csr=d["valid"], test_csr=d["test"], need_graph=False,
                             device=gpu_device, sample="pairwise", graph_source="train", seed=5)
    v = _victim(ds, gpu_device)
    (loss,) = v.train_step()
    assert np.isfinite(loss) and v.steps_done.tolist() == [(U - 1 + CFG["batch_size"] - 1) // CFG["batch_size"]]
    S = _score_matrix(v, [7, 7], gpu_device)
    assert np.all(np.isfinite(S)) and np.array_equal(_bits(S[0]), _bits(S[1]))
