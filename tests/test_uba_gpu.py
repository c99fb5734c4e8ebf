"""GPU tests of the UBA attacker (recad_amd/attack/uba.py over csrc/uba.hip and csrc/aush.hip): the inherited GAN against Aush bit
for bit, budget_matrix against the restatement on replayed draws, generate_fake's rows, and the defence workflow of the
reference's README with this package's names.  The kernels one entry point at a time are in tests/test_uba_kernels_gpu.py."""
import numpy as np
import pytest
import torch

from recad_amd import dataset, model, synth, workflow

from . import _uba_restate as R

pytestmark = pytest.mark.gpu
TARGET_USERS = [5, 17, 40, 41, 77, 120, 150, 199, 230, 256, 280, 299]


def _tiny(dev):
    d = synth.make("tiny")
    victim = dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], device=dev,
                                 graph_source="train", seed=5)
    r = synth.with_ratings(d)
    explicit = dataset.from_config("explicit", "tiny", train_csr=r["train"], valid_csr=r["valid"], test_csr=r["test"], device=dev)
    ptr, idx, val = (np.asarray(a) for a in r["train"])
    return victim, explicit, (ptr, idx, val)


def _most_rated(csr, n_items):
    return int(np.argmax(np.bincount(csr[1], minlength=n_items)))


def _uba(explicit, dev, csr, torch_seed=2023, **kw):
    cfg = dict(attack_num=len(TARGET_USERS), filler_num=8, seed=3, device=dev, target_user_ids=TARGET_USERS,
               selected_ids=[_most_rated(csr, explicit.n_items)])
    cfg.update(kw)
    torch.manual_seed(torch_seed)
    return model.from_config("attacker", "uba", **cfg).I(dataset=explicit)


def test_train_step_is_aush_bit_for_bit(gpu_device):
    _, explicit, csr = _tiny(gpu_device)
    u = _uba(explicit, gpu_device, csr)
    torch.manual_seed(2023)
    a = model.from_config("attacker", "aush", attack_num=len(TARGET_USERS), filler_num=8, seed=3, device=gpu_device,
                          selected_ids=u.selected_ids).I(dataset=explicit)
    # inherited unchanged: the very same functions (VarDim has no __eq__, so the descriptions are compared as printed)
    for name in ("train_step", "input_describe", "output_describe"):
        assert name not in vars(type(u)) and getattr(type(u), name) is getattr(type(a), name), name
    assert repr(u.input_describe()) == repr(a.input_describe()) and u.output_describe() == a.output_describe()
    for _ in range(2):
        assert u.train_step(target_id_list=[0]) == a.train_step(target_id_list=[0])
        assert np.array_equal(u.last_batch_losses, a.last_batch_losses)
    assert torch.equal(u.d_param, a.d_param) and torch.equal(u.g_w2, a.g_w2)


@pytest.mark.parametrize("hops", ["elementwise", "matrix"])
def test_budget_matrix_replay_and_own_draws(gpu_device, hops):
    _, explicit, (ptr, idx, val) = _tiny(gpu_device)
    u = _uba(explicit, gpu_device, (ptr, idx, val), hops=hops, budget=3, selected_ids=[62])
    mat = R.dense(explicit.n_users, explicit.n_items, ptr, idx, val)
    side_ptr, _ = R.side_layout(mat, TARGET_USERS, 62)
    assert np.array_equal(side_ptr, u.side_ptr) and u.scratch_bytes > 0
    draws = np.random.default_rng(4).integers(1, 6, size=(3, R.TRIALS, side_ptr[-1]))
    ref_prob, ref_ties, _, _ = R.prob(mat, TARGET_USERS, 62, 3, draws, hops)
    assert np.array_equal(u.replay_budget_matrix(draws), ref_prob) and u.last_tie_dependent == ref_ties
    p = u.budget_matrix()
    assert p.shape == (len(TARGET_USERS), 3) and p.dtype == np.float64 and np.array_equal(p * 10, np.round(p * 10)) and p.min() >= 0 and p.max() <= 1
    twin = _uba(explicit, gpu_device, (ptr, idx, val), hops=hops, budget=3, selected_ids=[62])
    assert np.array_equal(twin.budget_matrix(), p)           # one seed, one stream
    with pytest.raises(ValueError):
        u.replay_budget_matrix(np.zeros_like(draws))


def test_generate_fake_rows(gpu_device):
    _, explicit, (ptr, idx, val) = _tiny(gpu_device)
    u = _uba(explicit, gpu_device, (ptr, idx, val), hops="matrix")
    s, targets = u.selected_ids[0], [3, 11]
    before = [np.array(a) for a in explicit.rating_csr("train")]
    torch.manual_seed(1)
    fake = u.generate_fake(target_id_list=targets)
    chosen = u.last_templates
    assert fake.dtype == np.float32 and fake.shape == (len(chosen), explicit.n_items) and len(chosen) > 0
    assert set(chosen.tolist()) <= set(TARGET_USERS)
    assert (fake[:, targets] == 5).all()
    assert np.isin(fake[:, s], [1, 2, 3, 4, 5]).all()
    mat = R.dense(explicit.n_users, explicit.n_items, ptr, idx, val)
    rest = np.ones(explicit.n_items, dtype=bool)
    rest[targets + [s]] = False
    for r, user in enumerate(chosen):
        nz = np.nonzero(fake[r] * rest)[0]
        assert 1 <= len(nz) <= 8 and np.array_equal(fake[r, nz], mat[user, nz])      # the fillers are the template user's own ratings
    after = explicit.rating_csr("train")
    assert all(np.array_equal(b, np.asarray(a)) for b, a in zip(before, after))       # the dataset is not written
    assert np.array_equal(u._val.cpu().numpy(), val.astype(np.float32))


def test_defense_workflow_with_uba_and_pca_select_users(gpu_device):
    victim_data, explicit, csr = _tiny(gpu_device)
    attacker = model.from_config("attacker", "uba", attack_num=len(TARGET_USERS), filler_num=8, seed=3, device=gpu_device, hops="matrix",
                                 target_user_ids=TARGET_USERS, selected_ids=[_most_rated(csr, explicit.n_items)])
    wf = workflow.from_config("defense", victim_data=victim_data, attack_data=explicit, defense_data=explicit,
                              victim=model.from_config("victim", "lightgcn", latent_dim_rec=32, lightGCN_n_layers=2), attacker=attacker,
                              defender=model.from_config("defender", "PCASelectUsers", attack_num=15, device=gpu_device),
                              rec_epoch=2, attack_epoch=1, target_id_list=[0], device=gpu_device)
    res = wf.execute()
    assert wf.fake_dataset.n_users > victim_data.n_users and wf.defender.user_num == wf.fake_dataset.n_users
    for part in ("attacked", "defended"):
        assert "pred_shift" in res[part] and any(k.startswith("HR@") for k in res[part]), res
        assert all(np.isfinite(v) for v in res[part].values()), res
