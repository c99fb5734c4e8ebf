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
