"""GPU tests of the average, segment and bandwagon attackers (recad_amd/attack/heuristic.py over csrc/heuristic.hip): the
reference's own runs on the game data replayed through replay_fake (tests/golden/make_golden_heuristic.py) -- exact --, the
statistics read at .I() against the reference's within the float64 summation bound, the popularity rule, and the attack and
defence workflows end to end on the tiny synthetic shape.  The kernels one entry point at a time are in
tests/test_heuristic_kernels_gpu.py; the fixtures' two conditions are stated in tests/test_heuristic_host.py."""
import os

import numpy as np
import pytest

from recad_amd import dataset, model, synth, workflow
from recad_amd.defense.pca_select_users import flag_count

from . import _heuristic_restate as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("average", "segment", "bandwagon")


def _game(dev):
    p = np.load(os.path.join(GOLDEN, "aush_game_partial.npz"))
    return dataset.from_config("explicit", "game", train_dict=p["train_kvr"], valid_dict=p["valid_kvr"], test_dict=p["test_kvr"], device=dev)


def _profile(g, pre):
    ref = np.zeros(tuple(g[pre + "fake_shape"]), dtype=np.float32)
    ref[g[pre + "fake_rows"], g[pre + "fake_cols"]] = g[pre + "fake_vals"]
    return ref


@pytest.mark.parametrize("name,pre", [("average", "a_"), ("average", "b_"), ("segment", ""), ("bandwagon", "")])
def test_replay_of_the_reference_draws_is_exact(gpu_device, name, pre):
    g = np.load(os.path.join(GOLDEN, f"heur_game_{name}.npz"))
    ds = _game(gpu_device)
    kw = {"selected_ids": g[pre + "selected_ids"].tolist()} if name == "segment" else {}
    att = model.from_config("attacker", name, attack_num=int(g[pre + "attack_num"]), filler_num=int(g[pre + "filler_num"]), seed=1,
                            device=gpu_device, **kw).I(dataset=ds)
    assert att.n_items == int(g["n_items"])
    if name != "average":
        assert set(att.selected_ids) == set(g[pre + "selected_ids"].tolist())    # bandwagon: the popularity rule found them
    fake = att.replay_fake(g[pre + "cols"], g[pre + "vals"] if pre + "vals" in g else None, g[pre + "targets"].tolist())
    ref = _profile(g, pre)
    assert fake.dtype == np.float32 and fake.shape == ref.shape
    assert np.array_equal(fake, ref)
    assert att.output_describe()["generate_fake"]["fake_profile"] == (np.ndarray, ref.shape)
    assert set(att.input_describe()) == {"generate_fake"}


def test_statistics_and_popular_items_match_the_reference(gpu_device):
    g = np.load(os.path.join(GOLDEN, "heur_game_bandwagon.npz"))
    att = model.from_config("attacker", "bandwagon", seed=1, device=gpu_device).I(dataset=_game(gpu_device))
    n, mx = int(g["n_ratings"]), float(g["max_rating"])
    assert np.array_equal(att.item_count, g["item_count"]) and att.n_rated == int((g["item_count"] > 0).sum())
    assert np.all(np.abs(att.item_mean - g["item_mean"]) <= R.stat_bound(g["item_count"], mx))
    assert abs(att.global_mean - float(g["global_mean"])) <= R.stat_bound(n, mx)
    assert abs(att.global_std - float(g["global_std"])) <= R.stat_bound(n, mx)
    # the 11th and 12th largest counts differ (tests/test_heuristic_host.py), so the popular set is unique: ids as a set,
    # counts as a sequence, and this build's order among equal counts
    ids, counts = att.popular(11)
    assert att.selected_ids == ids and set(ids) == set(g["popular_ids"].tolist()) and counts == g["popular_counts"].tolist()
    r_ids, _ = R.popular(g["item_count"], 11)
    assert ids == r_ids.tolist()


def test_generate_fake_draws_a_fresh_stream_per_call(gpu_device):
    ds = _game(gpu_device)
    out = []
    for seed in (4, 4, 5):
        att = model.from_config("attacker", "average", attack_num=7, filler_num=5, seed=seed, device=gpu_device).I(dataset=ds)
        out.append((att.generate_fake(target_id_list=[3, 11]), att.generate_fake(target_id_list=[3, 11])))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert not np.array_equal(out[0][0], out[0][1]) and not np.array_equal(out[0][0], out[2][0])
    fake = out[0][0]
    assert fake.shape == (7, ds.n_items) and (fake[:3, 3] == 5).all() and (fake[3:6, 11] == 5).all() and not fake[6, [3, 11]].any()
    assert ((fake != 0).sum(axis=1) == [6, 6, 6, 6, 6, 6, 5]).all()
    for bad in (dict(target_id_list=[ds.n_items]), dict(target_id_list=[-1]), dict(target_id_list=[])):
        with pytest.raises(ValueError):
            att.generate_fake(**bad)
    with pytest.raises(ValueError):
        att.replay_fake([[1, 1, 2, 4, 5]], [[3.0] * 5], [3])                     # a repeated column
    with pytest.raises(ValueError):
        att.replay_fake([[1, 2, 3, 4, 5]], [[3.0] * 5], [3])                     # a target among the columns


# ---------------------------------------------------------------- workflows
def _tiny(dev):
    d = synth.make("tiny")
    victim = dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], device=dev,
                                 graph_source="train", seed=5)
    r = synth.with_ratings(d)
    explicit = dataset.from_config("explicit", "tiny", train_csr=r["train"], valid_csr=r["valid"], test_csr=r["test"], device=dev)
    return victim, explicit


def _attacker(name, dev):
    kw = {"selected_ids": [3, 50, 120]} if name == "segment" else {}
    return model.from_config("attacker", name, attack_num=15, filler_num=8, seed=3, device=dev, **kw)


def _finite(res):
    return all(_finite(v) if isinstance(v, dict) else np.isfinite(v) for v in res.values())


@pytest.mark.parametrize("name", NAMES)
def test_no_defense_workflow(gpu_device, name):
    victim_data, explicit = _tiny(gpu_device)
    wf = workflow.from_config("no defense", victim_data=victim_data, attack_data=explicit,
                              victim=model.from_config("victim", "lightgcn", latent_dim_rec=32, lightGCN_n_layers=2),
                              attacker=_attacker(name, gpu_device), rec_epoch=2, target_id_list=[0], device=gpu_device)
    res = wf.execute()
    assert res["n_eval_users"] > 0 and _finite(res)
    assert wf.fake_dataset.n_users == victim_data.n_users + 15


@pytest.mark.parametrize("name", NAMES)
def test_defense_workflow(gpu_device, name):
    victim_data, explicit = _tiny(gpu_device)
    wf = workflow.from_config("defense", victim_data=victim_data, attack_data=explicit, defense_data=explicit,
                              victim=model.from_config("victim", "lightgcn", latent_dim_rec=32, lightGCN_n_layers=2),
                              attacker=_attacker(name, gpu_device),
                              defender=model.from_config("defender", "PCASelectUsers", attack_num=15, device=gpu_device),
                              rec_epoch=2, target_id_list=[0], device=gpu_device)
    res = wf.execute()
    assert wf.fake_dataset.n_users == victim_data.n_users + 15 == wf.defender.user_num
    assert res["n_flagged"] == flag_count(15, victim_data.n_users + 15)
    assert _finite(res["attacked"]) and _finite(res["defended"])
