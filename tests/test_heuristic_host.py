"""CPU tests of the average, segment and bandwagon attackers (recad_amd/attack/heuristic.py): the registry and its defaults,
the lazy-init contract, the loud failure without a HIP device, and the float64 restatement the GPU tests compare against
(tests/_heuristic_restate.py) held to the reference's own runs on the game data (tests/golden/make_golden_heuristic.py):
statistics, popular items and the replayed profiles, plus two wrong variants the fixtures must tell apart.

Two conditions of the fixtures, asserted when they were recorded and again here: no recorded normal value lies within 2^-20
of a half-integer (np.round of it is then the same in any float64 restatement), and the 11th and 12th largest item counts
differ (the popular SET is unique; the reference's order among equal counts is an unstable sort's, so ids are compared as a
set and counts as a sequence)."""
import os

import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, model
from recad_amd.attack import heuristic as heur_mod
from recad_amd.utils import InstantiateFail, NotInstantiatedError

from . import _heuristic_restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("average", "segment", "bandwagon")
MODES = {"average": R.ITEM, "segment": R.ONES, "bandwagon": R.GLOBAL}
KVR = np.array([[0, 1, 4], [0, 3, 5], [2, 1, 2], [1, 0, 1], [2, 6, 5]], dtype=np.int64)


def game_csr():
    p = np.load(os.path.join(GOLDEN, "aush_game_partial.npz"))
    ds = dataset.from_config("explicit", "game", train_dict=p["train_kvr"], valid_dict=p["valid_kvr"], test_dict=p["test_kvr"], device="cpu")
    return ds.n_items, ds.rating_csr()


def golden_cases():
    """(name, fixture, key prefix) of the four recorded generate_fake runs."""
    out = []
    for name in NAMES:
        g = np.load(os.path.join(GOLDEN, f"heur_game_{name}.npz"))
        out += [(name, g, pre) for pre in (("a_", "b_") if name == "average" else ("",))]
    return out


def golden_profile(g, pre):
    ref = np.zeros(tuple(g[pre + "fake_shape"]), dtype=np.float32)
    ref[g[pre + "fake_rows"], g[pre + "fake_cols"]] = g[pre + "fake_vals"]
    return ref


def test_registry_and_defaults_equal_the_reference():
    assert set(NAMES) <= set(model.factories["attacker"])
    assert model.factories["attacker"]["average"] is heur_mod.AverageAttack
    assert model.factories["attacker"]["segment"] is heur_mod.SegmentAttack
    assert model.factories["attacker"]["bandwagon"] is heur_mod.BandwagonAttack
    # recad/default.py:136-158
    ref = {"average": {"attack_num": 50, "filler_num": 36},
           "segment": {"attack_num": 50, "filler_num": 36, "selected_ids": [1153, 2201, 1572, 836, 523, 849, 1171, 344, 857, 1213, 1535]},
           "bandwagon": {"attack_num": 50, "filler_num": 36, "selected_ids": []}}
    for name in NAMES:
        cfg = default.MODEL["attacker"][name]
        assert {k: cfg[k] for k in ref[name]} == ref[name]
        assert set(cfg) == set(ref[name]) | {"seed", "logging_level", "device"} and cfg["seed"] is None
    assert default.MODEL["attacker"]["random"]["attack_num"] == 50           # untouched
    assert (_lib.RK_HEUR_GLOBAL, _lib.RK_HEUR_ITEM, _lib.RK_HEUR_ONES) == (R.GLOBAL, R.ITEM, R.ONES)


@pytest.mark.parametrize("name", NAMES)
def test_lazy_contract_and_no_cpu_fallback(name, monkeypatch):
    lazy = model.from_config("attacker", name, filler_num=2, not_a_key=3)
    assert lazy.model_name == name and lazy._init_config["filler_num"] == 2 and "not_a_key" not in lazy._init_config
    for call in (lambda: lazy.generate_fake(target_id_list=[0]), lambda: lazy.replay_fake([[1, 2]], [[3.0, 3.0]], [0]),
                 lambda: lazy.input_describe(), lambda: lazy.output_describe(), lambda: lazy.popular(3)):
        with pytest.raises(NotInstantiatedError):
            call()
    again = lazy.reset(attack_num=7)
    assert again._init_config["attack_num"] == 7 and again._init_config["filler_num"] == 2
    with pytest.raises(ValueError):
        lazy.reset(nonsense=1)
    assert not hasattr(type(lazy), "train_step")                             # both workflows skip the attacker's training
    ds = dataset.from_config("explicit", "toy", device="cpu", train_dict=KVR)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(InstantiateFail, match="HIP"):
        lazy.I(dataset=ds)


def test_fixture_conditions():
    for name, g, pre in golden_cases():
        if pre + "vals" in g:
            v = g[pre + "vals"]
            assert np.abs(v - np.floor(v) - 0.5).min() > 2.0 ** -20, (name, pre)
        else:
            assert name == "segment"
        cols = g[pre + "cols"]
        assert cols.shape == (int(g[pre + "attack_num"]), int(g[pre + "filler_num"]))
        assert all(len(set(row)) == len(row) for row in cols.tolist())
        assert not np.isin(cols, np.concatenate([g[pre + "targets"], g[pre + "selected_ids"]])).any()
    g = np.load(os.path.join(GOLDEN, "heur_game_bandwagon.npz"))
    top = np.sort(g["item_count"])[::-1]
    assert top[10] != top[11] and top[11] == int(g["count_12th"]) and top[10] == g["popular_counts"].min()
    assert g["selected_ids"].tolist() == g["popular_ids"].tolist() and len(g["popular_ids"]) == 11


def test_restated_statistics_and_popular_items_match_the_reference():
    I, (ptr, idx, val) = game_csr()
    g = np.load(os.path.join(GOLDEN, "heur_game_average.npz"))
    assert I == int(g["n_items"]) and len(idx) == int(g["n_ratings"])        # no (user, item) pair is stored twice in game
    count, mean, gmean, gstd, n_rated = R.item_stats(I, idx, val)
    mx = float(g["max_rating"])
    assert np.array_equal(count, g["item_count"]) and n_rated == int((g["item_count"] > 0).sum())
    assert np.all(np.abs(mean - g["item_mean"]) <= R.stat_bound(count, mx))
    assert abs(gmean - float(g["global_mean"])) <= R.stat_bound(len(idx), mx)
    assert abs(gstd - float(g["global_std"])) <= R.stat_bound(len(idx), mx)
    ids, counts = R.popular(count, 11)
    assert set(ids.tolist()) == set(g["popular_ids"].tolist())
    assert counts.tolist() == g["popular_counts"].tolist()
    for a, b in zip(range(10), range(1, 11)):                                 # larger id first among equal counts
        assert counts[a] > counts[b] or ids[a] > ids[b]
    few_ids, few_counts = R.popular([0, 3, 0, 3, 1], 4)
    assert few_ids.tolist() == [3, 1, 4] and few_counts.tolist() == [3, 3, 1]


def test_restated_replay_equals_the_reference_profiles():
    I, _ = game_csr()
    for name, g, pre in golden_cases():
        x = g[pre + "vals"] if pre + "vals" in g else None
        got = R.profiles(int(g[pre + "attack_num"]), I, g[pre + "targets"].tolist(), g[pre + "selected_ids"].tolist(), g[pre + "cols"], x)
        assert np.array_equal(got, golden_profile(g, pre)), (name, pre)


def test_fixtures_reject_wrong_variants():
    """Target assignment by r % n_targets, and a rated item's own std as the scale of its normal value (the reference stores
    the MEAN there, heuristic.py:98): the recorded profiles differ from both."""
    I, (ptr, idx, val) = game_csr()
    g = np.load(os.path.join(GOLDEN, "heur_game_average.npz"))
    n, tg = int(g["b_attack_num"]), g["b_targets"].tolist()
    assert len(tg) == 2 and n % 2 == 1
    good = R.profiles(n, I, tg, [], g["b_cols"], g["b_vals"])
    bad = R.profiles(n, I, tg, [], g["b_cols"], g["b_vals"], variant="mod_targets")
    assert np.array_equal(good, golden_profile(g, "b_")) and not np.array_equal(bad, golden_profile(g, "b_"))
    assert (golden_profile(g, "b_")[n - 1, tg] == 0).all()                    # the remainder row rates no target
    # the standard normal behind every recorded value, under the reference's (loc, scale) = (mean, mean)
    count, mean, gmean, gstd, _ = R.item_stats(I, idx, val)
    cols, n = g["a_cols"], int(g["a_attack_num"])
    mu, sd = R.moments(R.ITEM, cols, gmean, gstd, mean, count)
    z = (g["a_vals"] - mu) / sd
    back = mu + sd * z
    assert np.abs(back - g["a_vals"]).max() < 2.0 ** -30                      # far inside the 2^-20 margin: rounding unchanged
    assert np.array_equal(R.profiles(n, I, g["a_targets"].tolist(), [], cols, back), golden_profile(g, "a_"))
    mu2, sd2 = R.moments(R.ITEM, cols, gmean, gstd, mean, count, variant="true_std", std=R.item_std(I, idx, val))
    wrong = R.profiles(n, I, g["a_targets"].tolist(), [], cols, mu2 + sd2 * z)
    assert (wrong != golden_profile(g, "a_")).sum() > cols.size // 10


def test_restated_draws_are_subsets_of_the_pool():
    for I, F, excl in ((64, 12, [3, 5, 63]), (9, 6, [0, 1, 8]), (5, 1, [2]), (300, 36, [])):
        c = R.draw_cols(7, (1 << 62) | 3, 40, F, I, excl)
        assert c.shape == (40, F) and c.min() >= 0 and c.max() < I and not np.isin(c, excl).any()
        assert all(len(set(row)) == F for row in c.tolist())
    full = R.draw_cols(1, 2, 5, 6, 9, [0, 1, 8])                               # filler_num = the pool: every pool item
    assert all(sorted(row) == [2, 3, 4, 5, 6, 7] for row in full.tolist())
    assert not np.array_equal(R.draw_cols(7, 1, 40, 12, 64, []), R.draw_cols(7, 2, 40, 12, 64, []))
    p = R.value_probs(3.6, 1.1)
    assert abs(p.sum() - 1) < 1e-12 and p.argmax() == 3 and R.value_probs(7.0, 0.0).tolist() == [0, 0, 0, 0, 1]


def test_generate_refuses_on_the_host_before_any_launch():
    """Every refusal of rk_heur_generate is decided from its host arguments, so it is visible without a device: the code comes
    back, with a message, and the (never dereferenced) device pointers are not touched."""
    import ctypes as C

    L, fake = _lib.lib(), C.c_void_p(64)

    def gen(n=7, I=65, F=5, tg=(3,), sel=(4,), mode=R.GLOBAL, cols=None, vals=None, stats=fake):
        t, s = (C.c_int32 * max(1, len(tg)))(*tg), (C.c_int32 * max(1, len(sel)))(*sel)
        return L.rk_heur_generate(n, I, F, t, len(tg), s if sel else None, len(sel), mode, 3.6, 1.1, stats, stats, cols, vals, 1, 0, fake, None)

    for kw in (dict(tg=[65]), dict(tg=[-1]), dict(sel=[65]), dict(F=0), dict(F=_lib.RK_HEUR_MAX_FILLER + 1), dict(F=64), dict(tg=[]),
               dict(tg=list(range(_lib.RK_HEUR_MAX_TARGETS + 1))), dict(sel=list(range(_lib.RK_HEUR_MAX_SELECT + 1))), dict(mode=3), dict(n=0),
               dict(vals=fake), dict(cols=fake), dict(mode=R.ITEM, stats=None), dict(I=1, tg=[0], sel=[], F=1, mode=R.ONES)):
        assert gen(**kw) == -22, kw
        assert L.rk_last_error()
    assert L.rk_heur_popular(5, fake, 0, fake, fake, C.byref(C.c_int32()), None) == -22
    assert L.rk_heur_item_stats(0, 0, None, None, fake, fake, fake, fake, None) == -22
