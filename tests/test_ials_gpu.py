"""GPU tests of the iALS victim end to end on a 300 x 120 synthetic dataset (d = 16, alpha = 40, lambda = 10, the item table drawn
from seed 7): five sweeps against the float64 sweeps of tests/_ials_restate.py, the returned loss against the dense objective, both
scoring paths, the batched evaluation and an EvalSession replay against the oracle's top-K, a constructed push attack through the
"no defense" workflow, a "defense" workflow with KnnSelectUsers, held-out quality, the state_dict round trip, reset(), the
repeatability of the fit and the refusal of a poisoned table."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from recad_amd import dataset, model, synth, workflow
from recad_amd.evaluate import EvalSession, eligible_users, full_catalog_topk, heldout_quality, hit_counts, quality_dict
from tests import _ials_restate as R
from tests import _rank_restate as RR

pytestmark = pytest.mark.gpu
U, I, D, ALPHA, LAM, SEED, SWEEPS = 300, 120, 16, 40.0, 10.0, 7, 5
TARGET, N_FAKE, N_POP = 85, 15, 5
EPS = 2.0 ** -52


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
                               device=dev, sample="pointwise", graph_source="train", seed=5)


def _lazy(**kw):
    return model.from_config("victim", "ials", **{"factor_num": D, "alpha": ALPHA, "reg_lambda": LAM, "seed": SEED, **kw})


def _victim(ds, dev, **kw):
    return _lazy(**kw).I(dataset=ds).to(dev)


def _train():
    ptr, idx = _data()["train"]
    return np.asarray(ptr).astype(np.int64), np.asarray(idx).astype(np.int64)


def _push_profile(idx):
    popular = np.argsort(-np.bincount(idx, minlength=I), kind="stable")[:N_POP + 1]
    popular = popular[popular != TARGET][:N_POP]
    return np.sort(np.r_[popular, [TARGET]])


@functools.lru_cache(maxsize=None)
def _reference(poisoned=False):
    """What is known without the device: the seeded item table, the float64 fit and the fp32 walk's fit of the train data (or of
    the data with the push profiles appended), and the walk's deviations that set the device's tolerances."""
    ptr, idx = _train()
    if poisoned:
        prof = _push_profile(idx)
        ptr, idx = np.r_[ptr, ptr[-1] + len(prof) * np.arange(1, N_FAKE + 1)], np.r_[idx, np.tile(prof, N_FAKE)]
    val = np.ones(len(idx), dtype=np.float32)
    Y0 = (torch.randn(I, D, generator=torch.Generator().manual_seed(SEED), dtype=torch.float32) * 0.01).numpy()
    X, Y = R.fit64(ptr, idx, val, I, Y0, ALPHA, LAM, SWEEPS)
    Xw, Yw = R.fit_walk(ptr, idx, val, I, Y0, ALPHA, LAM, SWEEPS)
    J = R.objective64(ptr, idx, val, I, X, Y, ALPHA, LAM)
    return {"ptr": ptr, "idx": idx, "val": val, "Y0": Y0, "X": X, "Y": Y, "J": J,
            "walk_tables": max(float(np.max(np.abs(Xw - X))), float(np.max(np.abs(Yw - Y)))),
            "walk_J": abs(R.objective64(ptr, idx, val, I, Xw, Yw, ALPHA, LAM) - J)}


def _tables(v):
    return v.user_emb.detach().cpu().numpy(), v.item_emb.detach().cpu().numpy()


def test_five_sweeps_against_float64(gpu_device):
    """Five train_steps from the seeded item table against five float64 sweeps from the same table.  The fp32 walk of the same
    sweeps ends 6.2e-6 from the float64 tables (max over both tables, whose entries reach 1.8) and 2.1e-4 from the float64
    objective 15643.3 (1.4e-8 of it); the device is allowed 4 x each and ends 5.3e-6 and 2.8e-4 away.  The returned loss is the dense objective of the tables read
    back, inside the J budget, and it does not rise from sweep to sweep by more than that budget."""
    ref = _reference()
    ds = _small(gpu_device)
    v = _victim(ds, gpu_device)
    assert np.array_equal(_bits(v.item_emb.cpu().numpy()), _bits(ref["Y0"])) and v.sweeps_done.tolist() == [0]
    assert next(v.parameters()).device.type == "cuda"
    ptr, idx, val = ref["ptr"], ref["idx"], ref["val"]
    last = None
    for sweep in range(SWEEPS):
        (loss,) = v.train_step(progress_bar=None)
        X, Y = _tables(v)
        J = R.objective64(ptr, idx, val, I, X, Y, ALPHA, LAM)
        budget = R.j_budget(ptr, idx, val, I, X, Y, ALPHA, LAM)
        print(f"sweep {sweep + 1}: loss {loss:.9e}, J / (U I) of the tables {J / (U * I):.9e}, |difference| {abs(loss * U * I - J):.3e}, budget {budget:.3e}")
        assert abs(loss * U * I - J) <= budget + 4 * EPS * J        # (the division and the product by U * I round once each)
        assert last is None or J <= last + budget, "the objective does not rise"
        last = J
    assert v.sweeps_done.tolist() == [SWEEPS]
    dev_tables = max(float(np.max(np.abs(X - ref["X"]))), float(np.max(np.abs(Y - ref["Y"]))))
    print(f"tables: device {dev_tables:.3e} from float64, walk {ref['walk_tables']:.3e}; J: device {abs(J - ref['J']):.3e}, walk {ref['walk_J']:.3e}")
    assert dev_tables <= 4 * ref["walk_tables"] and abs(J - ref["J"]) <= 4 * ref["walk_J"]


@functools.lru_cache(maxsize=None)
def _fitted(dev):
    ds = _small(dev)
    v = _victim(ds, dev)
    for _ in range(SWEEPS):
        v.train_step()
    return ds, v


def _restated_eval(S, users, targets, K):
    ptr, idx = _train()
    rows = [orc.topk_row(S[u], idx[ptr[u]:ptr[u + 1]], K, np.asarray(targets, dtype=np.int32)) for u in users]
    return [np.stack([r[j] for r in rows]) for j in range(4)]


def test_forward_equals_the_matrix_entries(gpu_device):
    """forward (rk_pair_scores: a wave sums the products of a pair) and the catalogue scores (the GEMM's k-ordered chain, which the
    oracle's score_rows restates) round differently: each lies within (d + 2) 2^-24 sum_k |x_k y_k| of the float64 entry."""
    ds, v = _fitted(gpu_device)
    X, Y = _tables(v)
    S64 = X.astype(np.float64) @ Y.astype(np.float64).T
    tol = (D + 2) * R.U24 * (np.abs(X).astype(np.float64) @ np.abs(Y).astype(np.float64).T)
    assert np.all(np.abs(orc.score_rows(X, Y) - S64) <= tol)
    rng = np.random.default_rng(3)
    users, items = rng.integers(0, U, size=700), rng.integers(0, I, size=700)
    pairs = v(torch.as_tensor(users, device=gpu_device), torch.as_tensor(items, device=gpu_device)).cpu().numpy()
    assert np.all(np.abs(pairs - S64[users, items]) <= tol[users, items]) and np.abs(pairs).max() > 0.1
    assert np.all(np.abs(pairs - orc.pair_scores(X, Y, users, items)) <= 2 * tol[users, items])
    again = v(torch.as_tensor(users, device=gpu_device), torch.as_tensor(items, device=gpu_device)).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(pairs))
    assert v(torch.zeros(0, dtype=torch.long, device=gpu_device), torch.zeros(0, dtype=torch.long, device=gpu_device)).numel() == 0


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
    assert sess._graph is not None, "the second run captured the evaluation"


class _PushAttack:
    """Test-local attacker: the constructed push, ratings of 5 so that inject_data(filter_num=4) keeps every item."""

    model_name = "push"

    def __init__(self, idx):
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
    """The push lifts HR@10 of item 85 from 0.007 to 0.142 under the float64 sweeps (289 eligible users); the fp32 fit may place a
    user whose margin is below the tables' deviation on the other side of rank 10, so the device's ratios are held to 0.02 of those."""
    ds = _small(gpu_device)
    _, idx = _train()
    topks = [5, 10, 20, 50]
    wf = workflow.from_config("no defense", victim_data=ds, attack_data=None, victim=_lazy(), attacker=_PushAttack(idx), rec_epoch=SWEEPS,
                              attack_epoch=0, device=gpu_device, target_id_list=[TARGET], topks=topks)
    res = wf.execute()
    assert len(wf.losses) == SWEEPS and all(a[0] >= b[0] for a, b in zip(wf.losses, wf.losses[1:])) and wf.fake_dataset.n_users == U + N_FAKE
    clean, poisoned = _reference(False), _reference(True)
    fp, fi = wf.fake_dataset.train_csr_sorted()
    assert np.array_equal(np.asarray(fp), poisoned["ptr"]) and np.array_equal(np.asarray(fi), poisoned["idx"]), "the same injected dataset"
    Xa, Ya = _tables(wf.fake_victim)
    assert max(np.max(np.abs(Xa - poisoned["X"])), np.max(np.abs(Ya - poisoned["Y"]))) <= 4 * poisoned["walk_tables"]
    before, n = R.hit_ratio(R.scores64(clean["X"], clean["Y"]), clean["ptr"], clean["idx"], TARGET, 10)
    after, n_after = R.hit_ratio(R.scores64(poisoned["X"], poisoned["Y"]), poisoned["ptr"], poisoned["idx"], TARGET, 10, real_users=U)
    print(f"HR@10 of item {TARGET} over {n} users: float64 {before:.3f} -> {after:.3f}, device {res['HR@10']:.3f} -> {res['HR@10 after attack']:.3f}")
    assert res["n_eval_users"] == n == n_after == 289 and after > before + 0.1
    assert abs(res["HR@10"] - before) <= 0.02 and abs(res["HR@10 after attack"] - after) <= 0.02
    assert res["HR@10 after attack"] > res["HR@10"] and res["pred_shift"] > 0


def test_defense_workflow_with_knn_defender(gpu_device):
    ds = _small(gpu_device)
    _, idx = _train()
    defender = model.from_config("defender", "KnnSelectUsers", k=25, attack_num=N_FAKE, device=gpu_device)
    wf = workflow.from_config("defense", victim_data=ds, attack_data=None, victim=_lazy(), attacker=_PushAttack(idx), defender=defender,
                              rec_epoch=2, attack_epoch=0, device=gpu_device, target_id_list=[TARGET], topks=[10, 20])
    res = wf.execute()
    assert set(res) == {"attacked", "defended", "n_flagged"} and wf.fake_dataset.n_users == U + N_FAKE
    assert wf.defended_victim.sweeps_done.tolist() == [2] and wf.defended_victim.num_users == wf.cleaned_dataset.n_users
    assert res["attacked"]["HR@10 after attack"] > res["attacked"]["HR@10"] == res["defended"]["HR@10"]
    assert wf.detection["n_fake"] == N_FAKE and 0 <= res["defended"]["HR@10 after attack"] <= 1


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
            assert abs(got[name] - r) <= (len(users) + 100) * EPS * abs(r), (split, name)
        assert 0 < got["Recall@10"] <= got["Recall@20"] <= 1


def test_state_dict_round_trip(gpu_device):
    ds, v = _fitted(gpu_device)
    state = {k: t.clone() for k, t in v.state_dict().items()}
    assert set(state) == {"user_emb", "item_emb", "user_bias", "item_bias", "sweeps_done"}
    fresh = _lazy(seed=SEED + 1).I(dataset=ds)
    fresh.load_state_dict({k: t.cpu() for k, t in state.items()})
    fresh = fresh.to(gpu_device)
    assert fresh.sweeps_done.tolist() == [SWEEPS]
    users = torch.arange(U, device=gpu_device).repeat_interleave(3)
    items = torch.arange(3 * U, device=gpu_device) % I
    assert torch.equal(v(users, items), fresh(users, items)) and bool(v(users, items).any())
    a, b = fresh.train_step(), _copy_of(v, ds, gpu_device).train_step()
    assert a == b and fresh.sweeps_done.tolist() == [SWEEPS + 1], "a loaded model goes on from where the saved one was"


def _copy_of(v, ds, dev):
    c = _lazy().I(dataset=ds).to(dev)
    c.load_state_dict(v.state_dict())
    return c


def test_reset_gives_an_untrained_model(gpu_device):
    ds, v = _fitted(gpu_device)
    lazy = v.reset()
    assert not lazy._is_instantiate and lazy._init_config["reg_lambda"] == LAM and lazy._init_config["seed"] == SEED
    again = lazy.I(dataset=ds).to(gpu_device)
    assert again.sweeps_done.tolist() == [0] and not again.user_emb.any()
    assert np.array_equal(_bits(again.item_emb.cpu().numpy()), _bits(_reference()["Y0"]))
    assert v.reset(factor_num=33, reg_lambda=3.0).I(dataset=ds).item_emb.shape == (I, 33)


def test_two_fits_from_one_seed_give_the_same_bits(gpu_device):
    ds = _small(gpu_device)
    a, b = _victim(ds, gpu_device), _victim(ds, gpu_device)
    la = [a.train_step() for _ in range(3)]
    lb = [b.train_step() for _ in range(3)]
    assert la == lb
    for s, t in zip(_tables(a), _tables(b)):
        assert np.array_equal(_bits(s), _bits(t)) and s.any()
    c = _victim(ds, gpu_device, seed=SEED + 1)
    c.train_step()
    assert not torch.equal(c.item_emb, a.item_emb)


def test_poisoned_table_is_refused_with_the_row(gpu_device):
    ds = _small(gpu_device)
    v = _victim(ds, gpu_device)
    v.train_step()
    before = [t.copy() for t in _tables(v)]
    item = 17
    with torch.no_grad():
        v.item_emb[item, 3] = float("nan")
    with pytest.raises(ValueError, match=r"rule 7 .*user row 0\b"):
        v.train_step()                    # the Gram matrix holds the NaN: every row is refused, the lowest is row 0
    assert v.sweeps_done.tolist() == [1], "a refused sweep is not counted"
    X, Y = _tables(v)
    assert np.array_equal(_bits(X), _bits(before[0])) and np.isnan(Y[item, 3]), "the tables are left as they were"
