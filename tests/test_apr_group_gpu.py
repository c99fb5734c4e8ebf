"""GPU tests of APR.train_group and of the "sweep" workflow on the 300 x 120 synthetic set of tests/test_apr_gpu.py (d = 16).  Every
grouped victim has a twin that is seeded identically (torch.manual_seed before .I(), the dataset's seed) and trained by its own
train_step loop; every comparison is exact."""
import numpy as np
import pytest
import torch

from recad_amd import dataset, model, synth, workflow
from recad_amd.evaluate import eligible_users, full_catalog_topk
from recad_amd.victim.apr import APR
from tests import test_apr_gpu as A

pytestmark = pytest.mark.gpu
U, I = A.U, A.I
N_FAKE = (0, 5, 10, 20)


def _poisoned(dev, n_fake, k):
    """the small set with n_fake injected users of 12 items each"""
    ds = A._small(dev)
    if not n_fake:
        return ds
    rng = np.random.default_rng(100 + k)
    fake = np.zeros((n_fake, I))
    for row in fake:
        row[rng.choice(I, size=12, replace=False)] = 5
    return ds.inject_data("explicit", fake, filter_num=4)


def _victims(dev, wrap=None):
    """four victims on sets with 0, 5, 10 and 20 injected users, adversarial from their second epoch on"""
    out = []
    for k, n_fake in enumerate(N_FAKE):
        ds = _poisoned(dev, n_fake, k)
        torch.manual_seed(20 + k)
        out.append(A._lazy(adv_start_epoch=1).I(dataset=wrap(k, ds) if wrap else ds).to(dev))
    return out


def _state(v):
    st = v.optimizer.state.get(v.weight, {})
    return {"weight": v.state_dict()["weight"].clone(), "epochs_done": v.state_dict()["epochs_done"].clone(),
            "exp_avg": st["exp_avg"].clone() if st else None, "exp_avg_sq": st["exp_avg_sq"].clone() if st else None,
            "step": float(st["step"]) if st else 0.0, "last_losses": None if v.last_losses is None else dict(v.last_losses),
            "sampler": repr(v.dataset._rng.bit_generator.state)}


def _same_state(a, b):
    sa, sb = _state(a), _state(b)
    for k in ("weight", "epochs_done", "exp_avg", "exp_avg_sq"):
        assert torch.equal(sa[k], sb[k]), k
    for k in ("step", "last_losses", "sampler"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])


def test_train_group_equals_train_step_to_the_bit(gpu_device):
    grouped, twins = _victims(gpu_device), _victims(gpu_device)
    assert [v.num_users for v in grouped] == [U + n for n in N_FAKE]
    losses = APR.train_group(grouped, epochs=3)
    alone = [[t.train_step()[0] for t in twins] for _ in range(3)]
    assert losses == alone and len(losses) == 3 and len(losses[0]) == 4
    for g, t in zip(grouped, twins):
        _same_state(g, t)
        assert g.epochs_done.tolist() == [3] and g.last_losses["adv"] > 0 and g._steps_done() > 3
        assert set(g.state_dict()) == {"weight", "epochs_done"}
    assert len({g._steps_done() for g in grouped}) > 1 or len({g.num_users for g in grouped}) == 4
    # the first epoch ran as BPR, the others with the adversarial term: a BPR-only twin differs
    bpr = _victims(gpu_device)[1]
    bpr.adv_start_epoch = 99
    for _ in range(3):
        bpr.train_step()
    assert not torch.equal(bpr.weight.data, grouped[1].weight.data)
    # one more epoch of each on its own still agrees, and so does a second group call
    for g, t in zip(grouped, twins):
        assert g.train_step() == t.train_step()
        _same_state(g, t)
    assert APR.train_group(grouped[::-1], epochs=1) == [[t.train_step()[0] for t in twins[::-1]]]
    for g, t in zip(grouped, twins):
        _same_state(g, t)
    # scoring
    g, t = grouped[2], twins[2]
    rng = np.random.default_rng(3)
    users = torch.as_tensor(rng.integers(0, U, size=500), device=gpu_device)
    items = torch.as_tensor(rng.integers(0, I, size=500), device=gpu_device)
    assert torch.equal(g(users, items), t(users, items))
    ptr, idx = g.dataset.train_csr_sorted()
    targets = np.array([A.TARGET, 0], dtype=np.int32)
    eu = eligible_users(ptr, idx, targets)
    ra, rb = (full_catalog_topk(v, eu, ptr, idx, targets, K=50) for v in (g, t))
    for k in ("top_ids", "top_scores", "target_score", "target_rank"):
        assert np.array_equal(ra[k], rb[k]), k


def test_a_bad_triplet_names_its_member_and_changes_no_victim(gpu_device):
    def wrap(k, ds):
        if k != 2:
            return ds
        bad = ds.generate_epoch()
        bad["negative_items"] = bad["negative_items"].clone()
        bad["negative_items"][77] = I
        return A._Recorded(ds, [bad])

    grouped = _victims(gpu_device, wrap)
    before = [v.weight.data.clone() for v in grouped]
    with pytest.raises(ValueError, match=r"member 2 .*rule 11 .*triplet 77\b"):
        APR.train_group(grouped, epochs=2)
    for v, w in zip(grouped, before):
        assert torch.equal(v.weight.data, w) and v.epochs_done.tolist() == [0] and v._steps_done() == 0 and v.last_losses is None
        st = v.optimizer.state.get(v.weight, {})
        assert not st or not (st["exp_avg"].any() or st["exp_avg_sq"].any())


# ------------------------------------------------------------------------------------------------------------ the workflow
def _sweep(dev, group, **kw):
    d = A._data()
    victim_data = A._small(dev)
    r = synth.with_ratings(dict(d, n_users=U, n_items=I), seed=7)
    explicit = dataset.from_config("explicit", "small", train_csr=r["train"], valid_csr=r["valid"], test_csr=r["test"], device=dev)
    cases = []
    for target in ([A.TARGET], [3]):
        cases.append({"attacker": workflow.RandomAttack(I, attack_num=10, filler_num=8, seed=1 + target[0]), "target_id_list": target})
        cases.append({"attacker": model.from_config("attacker", "average", attack_num=15, filler_num=8, seed=3, device=dev), "target_id_list": target})
    torch.manual_seed(5)
    return workflow.from_config("sweep", victim_data=victim_data, attack_data=explicit, victim=A._lazy(adv_start_epoch=1), cases=cases, rec_epoch=3,
                                attack_epoch=0, device=dev, topks=[5, 10, 20], group=group, **kw)


def test_sweep_grouped_equals_one_after_another(gpu_device):
    calls = []
    real = APR.train_group

    def counted(victims, **kw):
        calls.append(len(victims))
        return real(victims, **kw)

    out = {}
    for group in (3, 1):
        wf = _sweep(gpu_device, group, quality_split="test")
        try:
            APR.train_group = staticmethod(counted)
            res = wf.execute()
        finally:
            APR.train_group = staticmethod(real)
        out[group] = (res, wf)
        assert len(res) == 4 and [d.n_users for d in wf.fake_datasets] == [U + 10, U + 15, U + 10, U + 15]
        assert len(wf.losses) == 3 and wf.victim.epochs_done.tolist() == [3], "the clean victim is trained once"
        assert all(v.epochs_done.tolist() == [3] and v.last_losses["adv"] > 0 for v in wf.fake_victims)
        assert set(wf.timings) == {"train_clean_s", "train_poisoned_s", "evaluate_s"}
    assert calls == [3, 1], "group = 3 trains the four cases in chunks of 3 and 1, group = 1 never groups"
    (a, wa), (b, wb) = out[3], out[1]
    assert [list(r) for r in a] == [list(r) for r in b]
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert all(np.isfinite(v) for v in ra.values()), ra
        assert dict(ra) == dict(rb), (k, ra, rb)
        for name in ("Recall", "NDCG", "Precision", "HitRate", "MRR"):
            assert f"{name}@10" in ra and f"{name}@10 after attack" in ra
        assert ra["n_quality_users"] > 0 and ra["n_eval_users"] > 0
    assert wa.losses == wb.losses and wa.losses_fake == wb.losses_fake
    for va, vb in zip(wa.fake_victims, wb.fake_victims):
        assert torch.equal(va.weight.data, vb.weight.data)
    assert len(wa.timings["train_poisoned_s"]) == 2 and len(wb.timings["train_poisoned_s"]) == 4
