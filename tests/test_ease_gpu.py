"""GPU tests of the EASE victim end to end on the 300 x 200 synthetic dataset (lambda = 10): the fit against the float64 EASE
within the budgets of tests/_ease_restate.py, both scoring paths bit for bit against the restated chain over the device's own B,
the batched evaluation against the oracle's top-K applied to the restated rows, a constructed push attack through the "no defense"
workflow, a "defense" workflow with KnnSelectUsers, held-out quality, the state_dict round trip, reset() and the repeatability of
the fit."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from recad_amd import dataset, model, synth, workflow
from recad_amd.evaluate import eligible_users, full_catalog_topk, heldout_quality, quality_dict
from recad_amd.victim.ease import EASE
from tests import _ease_restate as R
from tests import _rank_restate as RR

pytestmark = pytest.mark.gpu
LAM, TARGET, N_FAKE, N_POP, I = 10.0, 139, 15, 5, 200
EPS = 2.0 ** -52


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tiny(dev):
    d = synth.make("tiny")
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], need_graph=False,
                               device=dev, sample="pointwise", graph_source="train", seed=5)


def _victim(ds, dev, **kw):
    return model.from_config("victim", "ease", **{"reg_lambda": LAM, **kw}).I(dataset=ds).to(dev)


@functools.lru_cache(maxsize=None)
def _train():
    d = synth.make("tiny")
    ptr, idx = (np.asarray(a) for a in d["train"])
    return ptr, idx.astype(np.int32)


def _push_profiles(idx):
    """15 x 200 ratings: each profile gives 5 stars to the target and to the 5 most rated items."""
    popular = np.argsort(-np.bincount(idx, minlength=I), kind="stable")[:N_POP + 1]
    popular = popular[popular != TARGET][:N_POP]
    fake = np.zeros((N_FAKE, I))
    fake[:, popular] = 5
    fake[:, TARGET] = 5
    return fake


@functools.lru_cache(maxsize=None)
def _reference(poisoned, block=0):
    """What is known without the device about the clean train data, or the data with the push profiles appended (as 0/1 rows, the
    way the implicit dataset stores them): X, A, P*, the walk's error and the budgets e_P, e_B."""
    ptr, idx = _train()
    X = R.dense(ptr, idx, np.ones(len(idx)), I)
    if poisoned:
        X = np.vstack([X, (_push_profiles(idx) > 0).astype(np.int64)])
    A = R.matrix(R.gram(X), LAM)
    P_star, kappa = R.inverse64(A)
    P_walk, bad = R.invert_walk(A, block)
    assert bad is None
    e_P = R.p_budget(float(np.max(np.abs(P_walk.astype(np.float64) - P_star))), I, kappa, P_star)
    return {"X": X, "A": A, "P_star": P_star, "e_P": e_P, "e_B": R.b_budget(e_P, P_star)}


def _B(v):
    return v.B.detach().cpu().numpy()


def _restated_eval(S, users, targets, K):
    """orc.topk_row on the restated rows: (top ids, top scores, target scores, target ranks)."""
    ptr, idx = _train()
    rows = [orc.topk_row(S[u], idx[ptr[u]:ptr[u + 1]], K, np.asarray(targets, dtype=np.int32)) for u in users]
    return [np.stack([r[j] for r in rows]) for j in range(4)]


def test_fit_and_both_scoring_paths(gpu_device):
    ds = _tiny(gpu_device)
    ref = _reference(False)
    v = _victim(ds, gpu_device)
    assert v.fitted.tolist() == [0] and next(v.parameters()).device.type == "cuda"
    assert v.train_step(progress_bar=None) == (0.0,) and v.fitted.tolist() == [1]
    B = _B(v)
    B_star = -(ref["P_star"] / np.diag(ref["P_star"])[None, :])
    np.fill_diagonal(B_star, 0.0)
    worst = float(np.max(np.abs(B - B_star) / np.maximum(ref["e_B"], 1e-300)))
    print(f"B: worst |error| / budget = {worst:.3f}, max |error| = {np.max(np.abs(B - B_star)):.3e}, max |B| = {np.max(np.abs(B_star)):.3f}")
    assert np.all(np.abs(B - B_star) <= ref["e_B"]) and np.all(_bits(np.diag(B)) == 0)
    # the scores: exactly the chain over the device's B, and within the budget of the float64 EASE
    S = R.scores(ref["X"], B, np.arange(300))
    out = torch.full((300 * I + 64,), float("nan"), device=gpu_device)
    v.score_matrix(torch.arange(300, dtype=torch.int32, device=gpu_device), out)
    got = out[: 300 * I].cpu().numpy().reshape(300, I)
    assert np.array_equal(_bits(got), _bits(S)) and bool(out[300 * I:].isnan().all())
    S_star = ref["X"].astype(np.float64) @ B_star
    e_S = R.score_budget(ref["X"], np.arange(300), ref["e_B"], ref["P_star"])
    print(f"scores: worst |error| / budget = {np.max(np.abs(got - S_star) / np.maximum(e_S, 1e-300)):.3f}, max |score| = {np.max(np.abs(S_star)):.3f}")
    assert np.all(np.abs(got - S_star) <= e_S) and np.max(np.abs(S_star)) > 0.1
    rng = np.random.default_rng(3)
    users, items = rng.integers(0, 300, size=700), rng.integers(0, I, size=700)
    pairs = v(torch.as_tensor(users, device=gpu_device), torch.as_tensor(items, device=gpu_device)).cpu().numpy()
    assert np.array_equal(_bits(pairs), _bits(S[users, items])) and pairs.any()
    assert v(torch.zeros(0, dtype=torch.long, device=gpu_device), torch.zeros(0, dtype=torch.long, device=gpu_device)).numel() == 0
    # train_step is a no-op once fitted; fit() rebuilds the same bits
    v.B.data.zero_()
    assert v.train_step() == (0.0,) and not v.B.any()
    assert v.fit() is v and np.array_equal(_bits(_B(v)), _bits(B)), "two fits of the same dataset give the same bits"
    # the other block width: fitted lazily by the first scoring call, inside the same budgets
    ref32 = _reference(False, 32)
    v2 = _victim(ds, gpu_device, block=32)
    out2 = torch.empty(300 * I, device=gpu_device)
    v2.score_matrix(torch.arange(300, dtype=torch.int32, device=gpu_device), out2)
    assert v2.fitted.tolist() == [1] and np.all(np.abs(_B(v2) - B_star) <= ref32["e_B"])
    assert np.array_equal(_bits(out2.cpu().numpy().reshape(300, I)), _bits(R.scores(ref["X"], _B(v2), np.arange(300))))


class _Mat:
    """A dataset that is only a rating matrix: what rating_csr() reads through info_describe()["train_mat"]."""

    def __init__(self, csr, n_users, n_items):
        self.csr, self.n_users, self.n_items = csr, n_users, n_items

    def info_describe(self):
        return {"n_users": self.n_users, "n_items": self.n_items, "train_mat": (*self.csr, self.n_items)}


def test_explicit_ratings(gpu_device):
    ptr, idx = _train()
    val = np.asarray(synth.with_ratings(synth.make("tiny"))["train"][2], dtype=np.float32)
    X = R.dense(ptr, idx, val, I)
    assert X.max() == 5
    v = _victim(_Mat((ptr, idx, val), 300, I), gpu_device, reg_lambda=500.0)
    users = torch.arange(0, 300, 7, dtype=torch.int32, device=gpu_device)
    out = torch.empty(users.numel() * I, device=gpu_device)
    v.score_matrix(users, out)
    A = R.matrix(R.gram(X), 500.0)
    P_star, kappa = R.inverse64(A)
    P_walk, _ = R.invert_walk(A, 0)
    e_B = R.b_budget(R.p_budget(float(np.max(np.abs(P_walk - P_star))), I, kappa, P_star), P_star)
    B_star = -(P_star / np.diag(P_star)[None, :])
    np.fill_diagonal(B_star, 0.0)
    assert np.all(np.abs(_B(v) - B_star) <= e_B)
    assert np.array_equal(_bits(out.cpu().numpy().reshape(-1, I)), _bits(R.scores(X, _B(v), users.cpu().numpy())))


def test_refusals_name_rule_and_index(gpu_device):
    ptr, idx = _train()
    bad = np.ones(len(idx), dtype=np.float32)
    bad[ptr[41] + 1] = 2.5
    v = _victim(_Mat((ptr, idx, bad), 300, I), gpu_device)
    with pytest.raises(ValueError, match=r"rule 1 .*row 41"):
        v.train_step()
    assert v.fitted.tolist() == [0]
    # 1041 users rate item 1 at 127: its squared norm passes 2^24 while every user norm is small
    n = 1041
    big = _Mat((np.arange(n + 1), np.ones(n, dtype=np.int32), np.full(n, 127, dtype=np.float32)), n, 3)
    v = _victim(big, gpu_device)
    with pytest.raises(ValueError, match=r"rule 5 .*item 1"):
        v.fit()
    assert v.fitted.tolist() == [0] and not v.B.any(), "A is untouched on that refusal"
    with pytest.raises(ValueError, match=r"rule 5 .*item 1"):
        v.train_step()            # still unfitted: the next call tries again


def test_full_catalog_topk_equals_the_oracle_on_restated_rows(gpu_device):
    ds = _tiny(gpu_device)
    v = _victim(ds, gpu_device)
    ptr, idx = ds.train_csr_sorted()
    targets = np.array([TARGET, 0], dtype=np.int32)
    users = eligible_users(ptr, idx, targets)
    assert 200 < len(users) < 300
    res = full_catalog_topk(v, users, ptr, idx, targets, K=100, chunk=128)     # three chunks
    S = R.scores(_reference(False)["X"], _B(v), np.arange(300))                  # the rows of the device's own B
    top_ids, top_scores, tscore, trank = _restated_eval(S, users, targets, 100)
    assert np.array_equal(_bits(res["top_scores"]), _bits(top_scores))
    assert np.array_equal(_bits(res["target_score"]), _bits(tscore)) and np.array_equal(res["target_rank"], trank)
    tie_free = np.array([len(np.unique(row)) == len(row) for row in top_scores])
    print(f"{int(tie_free.sum())} of {len(users)} rows have a tie-free top-100")
    assert tie_free.mean() > 0.5 and np.array_equal(res["top_ids"][tie_free], top_ids[tie_free])
    for r in np.nonzero(~tie_free)[0]:                                         # up to the first tie the ids are pinned too
        first = int(np.nonzero(np.diff(top_scores[r]) == 0)[0][0])
        assert np.array_equal(res["top_ids"][r, :first], top_ids[r, :first])


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
    _, _, tscore, trank = _restated_eval(S, users, [TARGET], 100)
    return {k: float(np.mean(trank[:, 0] < k)) for k in topks}, tscore[:, 0].astype(np.float64)


def test_push_attack_through_the_workflow(gpu_device):
    ds = _tiny(gpu_device)
    _, idx = _train()
    topks = [5, 10, 20, 50]
    wf = workflow.from_config("no defense", victim_data=ds, attack_data=None, victim=model.from_config("victim", "ease", reg_lambda=LAM),
                              attacker=_PushAttack(idx), rec_epoch=3, attack_epoch=0, device=gpu_device, target_id_list=[TARGET],
                              topks=topks)
    res = wf.execute()
    assert wf.losses == [(0.0,)] * 3 and wf.fake_dataset.n_users == 315
    clean, poisoned = _reference(False), _reference(True)
    fp, fi = wf.fake_dataset.train_csr_sorted()
    assert np.array_equal(R.dense(fp, fi, np.ones(len(fi)), I), poisoned["X"]), "the restatement runs on the same injected dataset"
    B_before, B_after = _B(wf.victim) if hasattr(wf, "victim") else None, _B(wf.fake_victim)
    assert np.all(np.abs(B_after + poisoned["P_star"] / np.diag(poisoned["P_star"])[None, :] * (1 - np.eye(I))) <= poisoned["e_B"])
    users = eligible_users(*ds.train_csr_sorted(), [TARGET])
    S_after = R.scores(poisoned["X"], B_after, np.arange(300))
    after, s1 = _restated_hr(S_after, users, topks)
    print(f"HR@10 of item {TARGET} over {len(users)} users: {res['HR@10']:.3f} before the push, {res['HR@10 after attack']:.3f} after")
    assert res["n_eval_users"] == len(users) == 294
    for k in topks:
        assert res[f"HR@{k} after attack"] == after[k], k
    if B_before is not None:
        before, s0 = _restated_hr(R.scores(clean["X"], B_before, np.arange(300)), users, topks)
        for k in topks:
            assert res[f"HR@{k}"] == before[k], k
        shift = float(np.mean(s1 - s0))
        assert abs(res["pred_shift"] - shift) <= 300 * EPS * float(np.mean(np.abs(s1) + np.abs(s0))) and shift > 0
    assert res["HR@10 after attack"] > res["HR@10"] and res["pred_shift"] > 0


def test_defense_workflow_with_knn_defender(gpu_device):
    ds = _tiny(gpu_device)
    _, idx = _train()
    defender = model.from_config("defender", "KnnSelectUsers", k=25, attack_num=N_FAKE, device=gpu_device)
    wf = workflow.from_config("defense", victim_data=ds, attack_data=None, victim=model.from_config("victim", "ease", reg_lambda=LAM),
                              attacker=_PushAttack(idx), defender=defender, rec_epoch=1, attack_epoch=0, device=gpu_device,
                              target_id_list=[TARGET], topks=[10, 20])
    res = wf.execute()
    assert set(res) == {"attacked", "defended", "n_flagged"} and wf.fake_dataset.n_users == 315
    assert wf.defended_victim.fitted.tolist() == [1] and wf.defended_victim.num_users == wf.cleaned_dataset.n_users
    assert res["attacked"]["HR@10 after attack"] > res["attacked"]["HR@10"] == res["defended"]["HR@10"]
    assert wf.detection["n_fake"] == N_FAKE and 0 <= res["defended"]["HR@10 after attack"] <= 1


def test_heldout_quality_equals_the_restated_lists(gpu_device):
    ds = _tiny(gpu_device)
    v = _victim(ds, gpu_device)
    topks = (10, 20)
    got = {split: heldout_quality(v, ds, split=split, topks=topks) for split in ("test", "valid")}
    S = R.scores(_reference(False)["X"], _B(v), np.arange(300))
    for split in ("test", "valid"):
        gt_ptr, gt_idx = ds.heldout_csr(split)
        users = np.nonzero(np.diff(gt_ptr))[0].astype(np.int32)
        top = _restated_eval(S, users, [], 20)[0]
        ref = quality_dict(RR.rank_metrics(top, users, gt_ptr, gt_idx, topks, RR.discount_table(20))[3], topks)
        assert got[split]["n_quality_users"] == ref["n_quality_users"] == len(users) > 0
        for name, r in ref.items():
            assert abs(got[split][name] - r) <= (len(users) + 100) * EPS * abs(r), (split, name)
        assert 0 < got[split]["Recall@10"] <= got[split]["Recall@20"] <= 1


def test_state_dict_round_trip_needs_no_refit(gpu_device, monkeypatch):
    ds = _tiny(gpu_device)
    v = _victim(ds, gpu_device)
    v.train_step()
    state = {k: t.clone() for k, t in v.state_dict().items()}
    assert set(state) == {"B", "fitted"}

    def no_fit(self):
        raise AssertionError("a loaded model must not be fitted again")

    fresh = model.from_config("victim", "ease", reg_lambda=LAM).I(dataset=ds)
    fresh.load_state_dict({k: t.cpu() for k, t in state.items()})
    fresh = fresh.to(gpu_device)
    monkeypatch.setattr(EASE, "fit", no_fit)
    users = torch.arange(300, dtype=torch.int32, device=gpu_device)
    a, b = torch.empty(300 * I, device=gpu_device), torch.empty(300 * I, device=gpu_device)
    v.score_matrix(users, a)
    fresh.score_matrix(users, b)
    assert torch.equal(a, b) and bool(a.any())
    assert fresh.train_step() == (0.0,)
    unfitted = _victim(ds, gpu_device)
    fresh.load_state_dict(unfitted.state_dict())
    with pytest.raises(AssertionError, match="fitted again"):
        fresh.train_step()        # an unfitted state makes the model unfitted again


def test_reset_gives_an_unfitted_model(gpu_device):
    ds = _tiny(gpu_device)
    v = _victim(ds, gpu_device)
    v.train_step()
    lazy = v.reset()
    assert not lazy._is_instantiate and lazy._init_config["reg_lambda"] == LAM
    again = lazy.I(dataset=ds).to(gpu_device)
    assert again.fitted.tolist() == [0] and not again.B.any()
    assert v.reset(reg_lambda=3.0, block=32).I(dataset=ds).B.shape == (I, I)


def test_two_fits_give_identical_weights(gpu_device):
    ds = _tiny(gpu_device)
    a, b = _victim(ds, gpu_device), _victim(ds, gpu_device)
    a.train_step()
    b.train_step()
    assert torch.equal(a.B.data, b.B.data) and bool(a.B.any())
    assert torch.equal(a.B.data.view(torch.int32), b.fit().B.data.view(torch.int32))
