"""GPU tests of the SLIM victim end to end on a 300 x 120 synthetic dataset (l1_reg = 1, l2_reg = 5, 50 sweeps): the fit through
the victim bit for bit against the numpy walk of tests/_slim_restate.py, both scoring paths bit for bit against the restated chain,
the batched evaluation against the oracle's top-K applied to the restated rows, a constructed push attack through the "no defense"
workflow, a "defense" workflow with KnnSelectUsers, held-out quality, the state_dict round trip, reset() and the repeatability of
the fit.  Nothing here has a tolerance: the walk is the only reference."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from recad_amd import dataset, model, synth, workflow
from recad_amd.evaluate import eligible_users, full_catalog_topk, heldout_quality, quality_dict
from recad_amd.victim.slim import SLIM
from tests import _rank_restate as RR
from tests import _slim_restate as R

pytestmark = pytest.mark.gpu
U, I, L1, L2, SWEEPS = 300, 120, 1.0, 5.0, 50
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
    return model.from_config("victim", "slim", **{"l1_reg": L1, "l2_reg": L2, "sweeps": SWEEPS, **kw})


def _victim(ds, dev, **kw):
    return _lazy(**kw).I(dataset=ds).to(dev)


def _train():
    ptr, idx = _data()["train"]
    return np.asarray(ptr).astype(np.int64), np.asarray(idx).astype(np.int32)


def _push_profiles(idx):
    """15 x 120 ratings: each profile gives 5 stars to the target and to the 5 most rated items."""
    popular = np.argsort(-np.bincount(idx, minlength=I), kind="stable")[:N_POP + 1]
    popular = popular[popular != TARGET][:N_POP]
    fake = np.zeros((N_FAKE, I))
    fake[:, popular] = 5
    fake[:, TARGET] = 5
    return fake


@functools.lru_cache(maxsize=None)
def _reference(poisoned=False, l1=L1, l2=L2, sweeps=SWEEPS):
    """The walk's fit of the clean train data, or of the data with the push profiles appended (as 0/1 rows, the way the implicit
    dataset stores them), and its score rows for the 300 real users."""
    ptr, idx = _train()
    X = R.dense(ptr, idx, np.ones(len(idx)), I)
    if poisoned:
        X = np.vstack([X, (_push_profiles(idx) > 0).astype(np.int64)])
    W, Rm, info = R.fit_walk(X, l1, l2, sweeps)
    return {"X": X, "W": W, "info": info, "S": R.scores(X, W, np.arange(U))}


def _W(v):
    return v.W.detach().cpu().numpy()


def _restated_eval(S, users, targets, K):
    """orc.topk_row on the restated rows: (top ids, top scores, target scores, target ranks)."""
    ptr, idx = _train()
    rows = [orc.topk_row(S[u], idx[ptr[u]:ptr[u + 1]], K, np.asarray(targets, dtype=np.int32)) for u in users]
    return [np.stack([r[j] for r in rows]) for j in range(4)]


def test_fit_and_both_scoring_paths(gpu_device):
    ds = _small(gpu_device)
    ref = _reference()
    v = _victim(ds, gpu_device)
    assert v.fitted.tolist() == [0] and next(v.parameters()).device.type == "cuda"
    assert v.train_step(progress_bar=None) == (0.0,) and v.fitted.tolist() == [1]
    W = _W(v)
    assert np.array_equal(_bits(W), _bits(ref["W"])), np.argwhere(_bits(W) != _bits(ref["W"]))[:5]
    assert np.all(_bits(np.diag(W)) == 0) and np.all(W >= 0) and 0.05 < (W > 0).mean() < 0.5, "sparse, non-negative, a zero diagonal"
    fi = v.fit_info()
    assert set(fi) == {"last_sweep", "support", "steps"} and all(t.dtype == torch.int32 and t.shape == (I,) and t.is_cuda for t in fi.values())
    for c, name in enumerate(("last_sweep", "support", "steps")):
        assert np.array_equal(fi[name].cpu().numpy(), ref["info"][:, c]), name
    print(f"fit: {int(fi['support'].sum())} positive weights, {int(fi['steps'].sum())} steps, last changing sweep {int(fi['last_sweep'].max())}")
    # the scores: exactly the chain over W
    out = torch.full((U * I + 64,), float("nan"), device=gpu_device)
    v.score_matrix(torch.arange(U, dtype=torch.int32, device=gpu_device), out)
    got = out[: U * I].cpu().numpy().reshape(U, I)
    assert np.array_equal(_bits(got), _bits(ref["S"])) and bool(out[U * I:].isnan().all()) and np.max(ref["S"]) > 0.1
    rng = np.random.default_rng(3)
    users, items = rng.integers(0, U, size=700), rng.integers(0, I, size=700)
    pairs = v(torch.as_tensor(users, device=gpu_device), torch.as_tensor(items, device=gpu_device)).cpu().numpy()
    assert np.array_equal(_bits(pairs), _bits(ref["S"][users, items])) and pairs.any(), "forward equals the matrix entries"
    assert v(torch.zeros(0, dtype=torch.long, device=gpu_device), torch.zeros(0, dtype=torch.long, device=gpu_device)).numel() == 0
    # train_step is a no-op once fitted; fit() rebuilds the same bits
    v.W.data.zero_()
    assert v.train_step() == (0.0,) and not v.W.any()
    assert v.fit() is v and np.array_equal(_bits(_W(v)), _bits(W)), "two fits of the same dataset give the same bits"
    # other settings, fitted lazily by the first scoring call
    ref2 = _reference(False, 0.0, 0.5, 3)
    v2 = _victim(ds, gpu_device, l1_reg=0, l2_reg=0.5, sweeps=3)
    out2 = torch.empty(U * I, device=gpu_device)
    v2.score_matrix(torch.arange(U, dtype=torch.int32, device=gpu_device), out2)
    assert v2.fitted.tolist() == [1] and np.array_equal(_bits(_W(v2)), _bits(ref2["W"]))
    assert np.array_equal(_bits(out2.cpu().numpy().reshape(U, I)), _bits(ref2["S"]))
    assert np.array_equal(v2.fit_info()["last_sweep"].cpu().numpy(), ref2["info"][:, 0]) and ref2["info"][:, 0].max() == 3


class _Mat:
    """A dataset that is only a rating matrix: what rating_csr() reads through info_describe()["train_mat"]."""

    def __init__(self, csr, n_users, n_items):
        self.csr, self.n_users, self.n_items = csr, n_users, n_items

    def info_describe(self):
        return {"n_users": self.n_users, "n_items": self.n_items, "train_mat": (*self.csr, self.n_items)}


def test_explicit_ratings_and_refusals(gpu_device):
    ptr, idx = _train()
    val = (1 + (np.arange(len(idx)) * 7) % 5).astype(np.float32)
    X = R.dense(ptr, idx, val, I)
    assert X.max() == 5
    v = _victim(_Mat((ptr, idx, val), U, I), gpu_device, l2_reg=50.0, sweeps=10)
    v.train_step()
    assert np.array_equal(_bits(_W(v)), _bits(R.fit_walk(X, L1, 50.0, 10)[0])) and v.W.any()
    bad = np.ones(len(idx), dtype=np.float32)
    bad[ptr[41] + 1] = 2.5
    v = _victim(_Mat((ptr, idx, bad), U, I), gpu_device)
    with pytest.raises(ValueError, match=r"rule 1 .*row 41"):
        v.train_step()
    assert v.fitted.tolist() == [0]
    # 1041 users rate item 1 at 127: its squared norm passes 2^24 while every user norm is small
    n = 1041
    big = _Mat((np.arange(n + 1), np.ones(n, dtype=np.int32), np.full(n, 127, dtype=np.float32)), n, 3)
    v = _victim(big, gpu_device)
    with pytest.raises(ValueError, match=r"rule 5 .*item 1"):
        v.fit()
    assert v.fitted.tolist() == [0] and not v.W.any()


def test_full_catalog_topk_equals_the_oracle_on_restated_rows(gpu_device):
    ds = _small(gpu_device)
    v = _victim(ds, gpu_device)
    ptr, idx = ds.train_csr_sorted()
    targets = np.array([TARGET, 0], dtype=np.int32)
    users = eligible_users(ptr, idx, targets)
    assert 200 < len(users) < U
    res = full_catalog_topk(v, users, ptr, idx, targets, K=50, chunk=128)      # three chunks
    top_ids, top_scores, tscore, trank = _restated_eval(_reference()["S"], users, targets, 50)
    assert np.array_equal(_bits(res["top_scores"]), _bits(top_scores))
    assert np.array_equal(_bits(res["target_score"]), _bits(tscore)) and np.array_equal(res["target_rank"], trank)
    tie_free = np.array([len(np.unique(row)) == len(row) for row in top_scores])
    print(f"{int(tie_free.sum())} of {len(users)} rows have a tie-free top-50")
    assert tie_free.mean() > 0.9 and np.array_equal(res["top_ids"], top_ids), "and a tie inside a row goes to the lower id"


class _PushAttack:
    """Test-local attacker: the constructed push, ratings of 5 so that inject_data(filter_num=4) keeps every item."""

    model_name = "push"

    def __init__(self, idx):
        self.fake = _push_profiles(idx)

    def I(self, **kw):
        return self

    def to(self, device):
        return self

    def input_describe(self):
        return {"generate_fake": {"target_id_list": (list, [])}}

    def generate_fake(self, target_id_list, **config):
        assert list(target_id_list) == [TARGET]
        return self.fake


def _restated_hr(S, users, topks):
    _, _, tscore, trank = _restated_eval(S, users, [TARGET], 50)
    return {k: float(np.mean(trank[:, 0] < k)) for k in topks}, tscore[:, 0].astype(np.float64)


def test_push_attack_through_the_workflow(gpu_device):
    """The push lifts HR@10 of item 85 from 0.000 to 0.090 over the 289 eligible users (HR@20 from 0.003 to 0.228): the device's
    ratios are the restated ones exactly, since W is."""
    ds = _small(gpu_device)
    _, idx = _train()
    topks = [5, 10, 20, 50]
    wf = workflow.from_config("no defense", victim_data=ds, attack_data=None, victim=_lazy(), attacker=_PushAttack(idx), rec_epoch=3,
                              attack_epoch=0, device=gpu_device, target_id_list=[TARGET], topks=topks)
    res = wf.execute()
    assert wf.losses == [(0.0,)] * 3 and wf.fake_dataset.n_users == U + N_FAKE
    clean, poisoned = _reference(False), _reference(True)
    fp, fi = wf.fake_dataset.train_csr_sorted()
    assert np.array_equal(R.dense(fp, fi, np.ones(len(fi)), I), poisoned["X"]), "the restatement runs on the same injected dataset"
    assert np.array_equal(_bits(_W(wf.fake_victim)), _bits(poisoned["W"]))
    users = eligible_users(*ds.train_csr_sorted(), [TARGET])
    after, s1 = _restated_hr(poisoned["S"], users, topks)
    before, s0 = _restated_hr(clean["S"], users, topks)
    print(f"HR@10 of item {TARGET} over {len(users)} users: {res['HR@10']:.3f} before the push, {res['HR@10 after attack']:.3f} after")
    assert res["n_eval_users"] == len(users) == 289
    for k in topks:
        assert res[f"HR@{k} after attack"] == after[k] and res[f"HR@{k}"] == before[k], k
    shift = float(np.mean(s1 - s0))
    assert abs(res["pred_shift"] - shift) <= 300 * EPS * float(np.mean(np.abs(s1) + np.abs(s0))) and shift > 0
    assert res["HR@10"] == 0.0 and res["HR@10 after attack"] > 0.08 and res["pred_shift"] > 0


def test_defense_workflow_with_knn_defender(gpu_device):
    ds = _small(gpu_device)
    _, idx = _train()
    defender = model.from_config("defender", "KnnSelectUsers", k=25, attack_num=N_FAKE, device=gpu_device)
    wf = workflow.from_config("defense", victim_data=ds, attack_data=None, victim=_lazy(), attacker=_PushAttack(idx), defender=defender,
                              rec_epoch=1, attack_epoch=0, device=gpu_device, target_id_list=[TARGET], topks=[10, 20])
    res = wf.execute()
    assert set(res) == {"attacked", "defended", "n_flagged"} and wf.fake_dataset.n_users == U + N_FAKE
    assert wf.defended_victim.fitted.tolist() == [1] and wf.defended_victim.num_users == wf.cleaned_dataset.n_users
    assert res["attacked"]["HR@10 after attack"] > res["attacked"]["HR@10"] == res["defended"]["HR@10"]
    assert wf.detection["n_fake"] == N_FAKE and 0 <= res["defended"]["HR@10 after attack"] <= 1


def test_heldout_quality_equals_the_restated_lists(gpu_device):
    ds = _small(gpu_device)
    v = _victim(ds, gpu_device)
    topks = (10, 20)
    S = _reference()["S"]
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


def test_state_dict_round_trip_needs_no_refit(gpu_device, monkeypatch):
    ds = _small(gpu_device)
    v = _victim(ds, gpu_device)
    v.train_step()
    state = {k: t.clone() for k, t in v.state_dict().items()}
    assert set(state) == {"W", "fitted"}

    def no_fit(self):
        raise AssertionError("a loaded model must not be fitted again")

    fresh = _lazy().I(dataset=ds)
    fresh.load_state_dict({k: t.cpu() for k, t in state.items()})
    fresh = fresh.to(gpu_device)
    monkeypatch.setattr(SLIM, "fit", no_fit)
    users = torch.arange(U, dtype=torch.int32, device=gpu_device)
    a, b = torch.empty(U * I, device=gpu_device), torch.empty(U * I, device=gpu_device)
    v.score_matrix(users, a)
    fresh.score_matrix(users, b)
    assert torch.equal(a, b) and bool(a.any())
    assert fresh.train_step() == (0.0,)
    unfitted = _victim(ds, gpu_device)
    fresh.load_state_dict(unfitted.state_dict())
    with pytest.raises(AssertionError, match="fitted again"):
        fresh.train_step()        # an unfitted state makes the model unfitted again


def test_reset_gives_an_unfitted_model(gpu_device):
    ds = _small(gpu_device)
    v = _victim(ds, gpu_device)
    v.train_step()
    lazy = v.reset()
    assert not lazy._is_instantiate and lazy._init_config["l1_reg"] == L1 and lazy._init_config["l2_reg"] == L2
    again = lazy.I(dataset=ds).to(gpu_device)
    assert again.fitted.tolist() == [0] and not again.W.any()
    assert v.reset(l1_reg=0.5, sweeps=3).I(dataset=ds).W.shape == (I, I)


def test_two_fits_give_identical_weights(gpu_device):
    ds = _small(gpu_device)
    a, b = _victim(ds, gpu_device), _victim(ds, gpu_device)
    a.train_step()
    b.train_step()
    assert torch.equal(a.W.data, b.W.data) and bool(a.W.any())
    assert torch.equal(a.W.data.view(torch.int32), b.fit().W.data.view(torch.int32))
    for name, t in a.fit_info().items():
        assert torch.equal(t, b.fit_info()[name]), name
