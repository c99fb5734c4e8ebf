"""GPU tests of the APR victim end to end on a 300 x 120 synthetic dataset (d = 16): five epochs over the device sampler's triplets
against the float64 replay of tests/_apr_restate.py on the same triplets, the reported losses, both scoring paths, the batched
evaluation and an EvalSession replay against the oracle's top-K, a constructed push through the "no defense" workflow, a "defense"
workflow with KnnSelectUsers, held-out quality, the state_dict round trip with the Adam moments, reset(), a foreign optimizer, and
the repeatability of a training run."""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from recad_amd import dataset, model, synth, workflow
from recad_amd.evaluate import EvalSession, eligible_users, full_catalog_topk, heldout_quality, hit_counts, quality_dict
from tests import _apr_restate as R
from tests import _rank_restate as RR

pytestmark = pytest.mark.gpu
U, I, D = 300, 120, 16
CFG = dict(factor_num=D, reg_lambda=1e-3, eps=0.5, adv_reg=1.0, adv_start_epoch=2, init_std=0.1, lr=0.01)
TARGET, N_FAKE, N_POP = 85, 15, 5
EPS64 = 2.0 ** -52


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


class _Recorded:
    """a dataset that hands out the epochs it is given, in turn and then again from the first (and records nothing itself)"""

    def __init__(self, ds, epochs):
        self.ds, self.epochs, self.at = ds, epochs, 0

    def __getattr__(self, name):
        return getattr(self.ds, name)

    def generate_epoch(self):
        ep = self.epochs[self.at % len(self.epochs)]
        self.at += 1
        return dict(ep)


@functools.lru_cache(maxsize=None)
def _epochs(dev, n=5):
    """n epochs of the device sampler: what train_step would have drawn"""
    ds = _small(dev)
    eps = [ds.generate_epoch() for _ in range(n)]
    for ep in eps:
        assert ep["batch_size"] == 1024 and ep["users"].numel() > 3000 and ep["users"].is_cuda
    return ds, eps


def _n_steps(eps):
    return sum((ep["users"].numel() + 1023) // 1024 for ep in eps)


def _host_epochs(eps):
    return [tuple(ep[k].cpu().numpy() for k in ("users", "positive_items", "negative_items")) for ep in eps]


def _lazy(**kw):
    return model.from_config("victim", "apr", **{**CFG, **kw})


def _victim(ds, dev, seed=11, **kw):
    torch.manual_seed(seed)
    return _lazy(**kw).I(dataset=ds).to(dev)


def _tables(v):
    return v.embedding_user.cpu().numpy(), v.embedding_item.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(dev):
    """the float64 replay and the plain fp32 numpy replay of the five recorded epochs from the seeded table"""
    ds, eps = _epochs(dev)
    torch.manual_seed(11)
    tab0 = (torch.randn(U + I, D) * CFG["init_std"]).numpy()
    kw = dict(batch=1024, U=U, lam=CFG["reg_lambda"], eps=CFG["eps"], adv_reg=CFG["adv_reg"], adv_start=CFG["adv_start_epoch"], lr=CFG["lr"])
    t64, h64 = R.replay(tab0, _host_epochs(eps), fp32=False, **kw)
    t32, h32 = R.replay(tab0, _host_epochs(eps), fp32=True, **kw)
    return {"tab0": tab0, "t64": t64, "h64": h64, "walk_tables": float(np.max(np.abs(t32 - t64))), "walk_hist": np.abs(h32 - h64)}


def test_five_epochs_against_float64(gpu_device):
    """Five train_steps over the recorded epochs (adversarial from the third on) against the float64 replay of the same triplets.
    The device may end 4 x as far from float64 as the plain fp32 numpy replay does, plus 2^-23 max|table|; the reported losses
    likewise, plus the loss budget of one step.

    Measured on the MI355X: the numpy replay ends 5.755e-07 from float64, the allowance is 2.353e-06, the device ends 4.676e-07 away
    (0.20 of the allowance) and its losses within 1.5e-9 (allowed 2e-6).  This test is why apr_coef_kernel works x and c out in
    double: with x and c in fp32 every stage of a step was inside its budget and the tables still ended 4.275e-06 away, because
    Adam divides by sqrt(v) and, over the first steps, turns a last-bit error of c into a large relative change of the update of
    an element with a small gradient history."""
    ref = _reference(gpu_device)
    ds, eps = _epochs(gpu_device)
    v = _victim(_Recorded(ds, eps), gpu_device)
    assert np.array_equal(_bits(v.weight.data.cpu().numpy()), _bits(ref["tab0"])) and v.epochs_done.tolist() == [0]
    for ep in range(5):
        (loss,) = v.train_step(progress_bar=None)
        got = np.array([v.last_losses[k] for k in ("bpr", "adv", "reg")])
        adv = CFG["adv_reg"] if ep >= CFG["adv_start_epoch"] else 0.0
        budget = 4 * ref["walk_hist"][ep] + (4 + D + 32) * R.U32 * np.abs(ref["h64"][ep]) + R.U32
        print(f"epoch {ep}: device {got}, float64 {ref['h64'][ep]}, |difference| {np.abs(got - ref['h64'][ep])}, allowed {budget}")
        assert np.all(np.abs(got - ref["h64"][ep]) <= budget)
        assert abs(loss - (got[0] + adv * got[1] + got[2])) <= 4 * EPS64 * abs(loss) and (got[1] > 0) == (adv > 0)
    assert v.epochs_done.tolist() == [5] and v._steps_done() == _n_steps(eps)
    tab = v.weight.data.cpu().numpy()
    dev_tables = float(np.max(np.abs(tab - ref["t64"])))
    allowed = 4 * ref["walk_tables"] + 2.0 ** -23 * float(np.abs(ref["t64"]).max())
    print(f"tables: device {dev_tables:.3e} from float64, walk {ref['walk_tables']:.3e}, allowed {allowed:.3e}, ratio {dev_tables / allowed:.3f}")
    assert dev_tables <= allowed


@functools.lru_cache(maxsize=None)
def _fitted(dev):
    ds, eps = _epochs(dev)
    v = _victim(_Recorded(ds, eps), dev)
    for _ in range(5):
        v.train_step()
    return ds, v


def _restated_eval(S, users, targets, K):
    ptr, idx = (np.asarray(a).astype(np.int64) for a in _data()["train"])
    rows = [orc.topk_row(S[u], idx[ptr[u]:ptr[u + 1]], K, np.asarray(targets, dtype=np.int32)) for u in users]
    return [np.stack([r[j] for r in rows]) for j in range(4)]


def test_forward_equals_the_table_dots(gpu_device):
    ds, v = _fitted(gpu_device)
    X, Y = _tables(v)
    S64 = X.astype(np.float64) @ Y.astype(np.float64).T
    tol = (D + 2) * R.U32 * (np.abs(X).astype(np.float64) @ np.abs(Y).astype(np.float64).T)
    rng = np.random.default_rng(3)
    users, items = rng.integers(0, U, size=700), rng.integers(0, I, size=700)
    pairs = v(torch.as_tensor(users, device=gpu_device), torch.as_tensor(items, device=gpu_device)).cpu().numpy()
    assert np.all(np.abs(pairs - S64[users, items]) <= tol[users, items]) and np.abs(pairs).max() > 0.01
    again = v(torch.as_tensor(users, device=gpu_device), torch.as_tensor(items, device=gpu_device)).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(pairs))
    ue, ie, ub, ib, mean = v.scoring_tables()
    assert mean == 0.0 and not ub.any() and not ib.any() and ue.data_ptr() == v.weight.data_ptr() and ie.shape == (I, D)
    assert v.scoring_tables_key() == v.scoring_tables_key()


def test_topk_and_eval_session_equal_the_oracle_and_each_other(gpu_device):
    ds, v = _fitted(gpu_device)
    ptr, idx = ds.train_csr_sorted()
    targets = np.array([TARGET, 0], dtype=np.int32)
    users = eligible_users(ptr, idx, targets)
    topks, K = (5, 10, 20, 50), 50
    assert 200 < len(users) < U
    res = full_catalog_topk(v, users, ptr, idx, targets, K=K, chunk=128)         # three chunks
    S = orc.score_rows(*_tables(v))
    top_ids, top_scores, tscore, trank = _restated_eval(S, users, targets, K)
    assert np.array_equal(_bits(res["top_scores"]), _bits(top_scores))
    assert np.array_equal(_bits(res["target_score"]), _bits(tscore)) and np.array_equal(res["target_rank"], trank)
    tie_free = np.array([len(np.unique(row)) == len(row) for row in top_scores])
    assert tie_free.mean() > 0.9 and np.array_equal(res["top_ids"][tie_free], top_ids[tie_free])
    sess = EvalSession(v, users, ptr, idx, targets, K=K, topks=topks, chunk=128)
    ref = full_catalog_topk(v, users, ptr, idx, targets, K=K, chunk=128, to_host=False)
    for round_ in range(3):                                                      # eager, captured, replayed
        got = {k: t.clone() for k, t in sess.run().items()}
        for k in ("top_ids", "top_scores", "target_score", "target_rank"):
            assert torch.equal(got[k], ref[k]), (round_, k)
        assert torch.equal(got["hit_counts"], hit_counts(ref["target_rank"], topks)), round_


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


@pytest.mark.parametrize("name,adv_reg", [("bpr", 0.0), ("apr", 1.0)])
def test_push_attack_through_the_workflow(gpu_device, name, adv_reg):
    """What the float64 run of tests/test_apr_host.py supports, and no more: the constructed push lifts HR@10 of the target, for
    BPR and for APR (40 epochs at lr 0.01 from the 0.01 initialisation, lambda 1e-4, adversarial from epoch 20).  Measured on the
    device: 0.003 -> 0.114 as BPR, 0.000 -> 0.104 as APR, over the 289 eligible users.  No robustness claim is made."""
    ds = _small(gpu_device)
    torch.manual_seed(5)
    lazy = _lazy(adv_reg=adv_reg, adv_start_epoch=20, init_std=0.01, reg_lambda=1e-4)
    wf = workflow.from_config("no defense", victim_data=ds, attack_data=None, victim=lazy, attacker=_PushAttack(), rec_epoch=40,
                              attack_epoch=0, device=gpu_device, target_id_list=[TARGET], topks=[5, 10, 20, 50])
    res = wf.execute()
    assert len(wf.losses) == 40 and wf.fake_dataset.n_users == U + N_FAKE and wf.fake_victim.epochs_done.tolist() == [40]
    assert (wf.fake_victim.last_losses["adv"] > 0) == (adv_reg > 0)
    print(f"PUSH {name}: HR@10 of item {TARGET} over {res['n_eval_users']} users {res['HR@10']:.3f} -> {res['HR@10 after attack']:.3f}")
    assert res["n_eval_users"] == 289
    assert res["HR@10 after attack"] > res["HR@10"]


def test_defense_workflow_with_knn_defender(gpu_device):
    ds = _small(gpu_device)
    defender = model.from_config("defender", "KnnSelectUsers", k=25, attack_num=N_FAKE, device=gpu_device)
    wf = workflow.from_config("defense", victim_data=ds, attack_data=None, victim=_lazy(), attacker=_PushAttack(), defender=defender,
                              rec_epoch=3, attack_epoch=0, device=gpu_device, target_id_list=[TARGET], topks=[10, 20])
    res = wf.execute()
    assert set(res) == {"attacked", "defended", "n_flagged"} and wf.fake_dataset.n_users == U + N_FAKE
    assert wf.defended_victim.epochs_done.tolist() == [3] and wf.defended_victim.num_users == wf.cleaned_dataset.n_users
    assert wf.defended_victim.last_losses["adv"] > 0, "the third epoch is adversarial"
    assert wf.detection["n_fake"] == N_FAKE
    for part in ("attacked", "defended"):
        assert 0 <= res[part]["HR@10"] <= 1 and 0 <= res[part]["HR@10 after attack"] <= 1


def test_heldout_quality_equals_the_restated_lists(gpu_device):
    ds, v = _fitted(gpu_device)
    topks = (10, 20)
    S = orc.score_rows(*_tables(v))
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


def test_state_dict_round_trip_with_the_adam_moments(gpu_device):
    ds, v = _fitted(gpu_device)
    state = {k: t.clone() for k, t in v.state_dict().items()}
    opt = copy.deepcopy(v.optimizer.state_dict())
    assert set(state) == {"weight", "epochs_done"} and state["epochs_done"].tolist() == [5]
    assert opt["state"][0]["exp_avg"].shape == (U + I, D) and bool(opt["state"][0]["exp_avg"].any()) and int(opt["state"][0]["step"]) == _n_steps(_epochs(gpu_device)[1])
    _, eps = _epochs(gpu_device)
    fresh = _lazy().I(dataset=_Recorded(ds, eps[:1]))
    fresh.load_state_dict({k: t.cpu() for k, t in state.items()})
    fresh.optimizer.load_state_dict(opt)
    fresh = fresh.to(gpu_device)
    assert fresh.epochs_done.tolist() == [5] and torch.equal(fresh.weight.data, v.weight.data)
    twin = _lazy().I(dataset=_Recorded(ds, eps[:1])).to(gpu_device)
    twin.load_state_dict(v.state_dict())
    twin.optimizer.load_state_dict(copy.deepcopy(v.optimizer.state_dict()))
    a, b = fresh.train_step(), twin.train_step()
    assert a == b and torch.equal(fresh.weight.data, twin.weight.data), "a loaded model goes on from where the saved one was"
    assert fresh.epochs_done.tolist() == [6] and fresh._steps_done() == _n_steps(eps) + _n_steps(eps[:1]) and fresh.last_losses["adv"] > 0
    cold = _lazy().I(dataset=_Recorded(ds, eps[:1])).to(gpu_device)
    cold.load_state_dict(v.state_dict())
    cold.train_step()
    assert not torch.equal(cold.weight.data, twin.weight.data), "without the moments the step differs"


def test_reset_gives_an_untrained_model(gpu_device):
    ds, v = _fitted(gpu_device)
    lazy = v.reset()
    assert not lazy._is_instantiate and lazy._init_config["eps"] == CFG["eps"]
    torch.manual_seed(11)
    again = lazy.I(dataset=ds).to(gpu_device)
    assert again.epochs_done.tolist() == [0] and again._steps_done() == 0
    assert np.array_equal(_bits(again.weight.data.cpu().numpy()), _bits(_reference(gpu_device)["tab0"]))
    assert v.reset(factor_num=33).I(dataset=ds).weight.shape == (U + I, 33)


def test_a_foreign_optimizer_steps_on_the_restated_gradients(gpu_device):
    """SGD through _unfused_epoch (the library returns each minibatch's dense gradient, torch steps): two epochs, the second
    adversarial, against the float64 replay with p -= lr g, under the idiom of the five-epoch test."""
    ds, eps = _epochs(gpu_device)
    kw = dict(batch=1024, U=U, lam=CFG["reg_lambda"], eps=CFG["eps"], adv_reg=CFG["adv_reg"], adv_start=1, lr=0.5, opt="sgd")
    tab0 = _reference(gpu_device)["tab0"]
    t64, h64 = R.replay(tab0, _host_epochs(eps[:2]), fp32=False, **kw)
    t32, _ = R.replay(tab0, _host_epochs(eps[:2]), fp32=True, **kw)
    v = _victim(_Recorded(ds, eps), gpu_device, optim="SGD", lr=0.5, adv_start_epoch=1)
    assert not v._fused_adam
    for ep in range(2):
        (loss,) = v.train_step()
        assert abs(loss - (h64[ep][0] + (ep >= 1) * h64[ep][1] + h64[ep][2])) <= 1e-4 * abs(loss)
    tab = v.weight.data.cpu().numpy()
    dev, walk = float(np.max(np.abs(tab - t64))), float(np.max(np.abs(t32 - t64)))
    print(f"SGD tables: device {dev:.3e} from float64, walk {walk:.3e}")
    assert np.abs(t64 - tab0).max() > 1e-3 and dev <= 4 * walk + 2.0 ** -23 * float(np.abs(t64).max())
    assert v.epochs_done.tolist() == [2] and v._steps_done() == 0


def test_two_trainings_from_one_seed_give_the_same_bits(gpu_device):
    out = []
    for _ in range(2):
        ds = _small(gpu_device)
        v = _victim(ds, gpu_device, seed=3)
        losses = [v.train_step() for _ in range(4)]
        out.append((losses, v.weight.data.cpu().numpy(), dict(v.last_losses)))
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2] and out[0][2]["adv"] > 0
    assert np.array_equal(_bits(out[0][1]), _bits(out[1][1])) and out[0][1].any()


def test_a_bad_triplet_is_refused_with_its_rule(gpu_device):
    ds, eps = _epochs(gpu_device)
    bad = dict(eps[0])
    bad["negative_items"] = bad["negative_items"].clone()
    bad["negative_items"][77] = I
    v = _victim(_Recorded(ds, [bad]), gpu_device)
    before = v.weight.data.clone()
    with pytest.raises(ValueError, match=r"rule 11 .*triplet 77\b"):
        v.train_step()
    assert torch.equal(v.weight.data, before) and v.epochs_done.tolist() == [0] and v._steps_done() == 0
