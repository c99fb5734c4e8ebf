"""CPU tests of the grouped APR training's host side: the "sweep" workflow's defaults, registration and plumbing (with a stub victim
that has no train_group, and with a counting one), every host-side refusal of APR.train_group raised before any device call, and
the ctypes prototype of rk_apr_train_epoch_group against the header."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from recad_amd import _lib, dataset, default, model, synth, workflow
from recad_amd.victim.apr import APR
from tests.test_host_logic import _StubVictim


def _tiny(**kw):
    d = synth.make("tiny")
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"], need_graph=False,
                               device=torch.device("cpu"), seed=5, **kw)


def _apr(ds=None, **kw):
    return model.from_config("victim", "apr", **{"factor_num": 4, **kw}).I(dataset=_tiny() if ds is None else ds)


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device call was made before the refusal")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "require_gpu", refuse)


# ------------------------------------------------------------------------------------------------------------ the C entry
def test_group_entry_prototype_matches_the_header():
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "recad_hip.h")).read()
    assert f"#define RK_APR_MAX_GROUP {_lib.RK_APR_MAX_GROUP}" in header and _lib.RK_APR_MAX_GROUP == 64
    assert "rk_apr_train_epoch_group" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 11 and "#define RK_ABI_VERSION 11" in header, "an entry was added, nothing changed"
    m = re.search(r"\bint rk_apr_train_epoch_group\(([^;]*)\);", header)
    assert m, "the header does not declare the entry"
    params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).replace("\n", " ").split(",")]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    types = [re.sub(r"\s+", " ", p[: -len(n)]).strip() for p, n in zip(params, names)]
    assert names == ["n_rep", "descs", "users", "pos", "neg", "n", "batch", "adam_t0", "apply_update", "losses", "status", "stream"]
    ptrs, dev = C.POINTER(C.c_void_p), C.c_void_p
    want = {"int32_t": C.c_int32, "const rk_apr_desc *": C.POINTER(_lib.AprDesc), "const int64_t *const *": ptrs, "double *const *": ptrs,
            "const int64_t *": C.POINTER(C.c_int64), "const int32_t *": C.POINTER(C.c_int32), "int32_t *": dev, "void *": dev}
    assert [want[t] for t in types] == list(_lib._SIGNATURES["rk_apr_train_epoch_group"])
    single = re.search(r"\bint rk_apr_train_epoch\(([^;]*)\);", header)
    assert single and len(single.group(1).split(",")) == len(_lib._SIGNATURES["rk_apr_train_epoch"]) == 11, "the single entry is as it was"


# ------------------------------------------------------------------------------------------------------------ train_group
def test_train_group_host_side_refusals_need_no_library(no_library):
    a, b = _apr(), _apr()
    with pytest.raises(ValueError, match="empty"):
        APR.train_group([])
    for bad in (object(), _StubVictim(), None, model.from_config("victim", "apr", factor_num=4)):      # the last is a lazy APR
        with pytest.raises(ValueError, match="member 1 .*expected an instantiated APR"):
            APR.train_group([a, bad])
    with pytest.raises(ValueError, match="member 2 is in the group twice"):
        APR.train_group([a, b, a])
    with pytest.raises(ValueError, match="member 1 has factor_num = 8, member 0 has 4"):
        APR.train_group([a, _apr(factor_num=8)])
    other = _tiny()
    other.config["pairwise_batch_size"] = a.dataset.config["pairwise_batch_size"] // 2
    with pytest.raises(ValueError, match="member 1 trains in minibatches of"):
        APR.train_group([a, _apr(other)])
    with pytest.raises(ValueError, match="member 1 is on the device meta"):
        APR.train_group([a, _apr().to("meta")])
    with pytest.raises(ValueError, match="member 1 has the optimizer SGD"):
        APR.train_group([a, _apr(optim="SGD")])
    ds = _tiny()
    many = [_apr(ds, factor_num=1) for _ in range(_lib.RK_APR_MAX_GROUP + 1)]
    with pytest.raises(ValueError, match="65 victims, at most 64"):
        APR.train_group(many)
    for epochs in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="epochs"):
            APR.train_group([a, b], epochs=epochs)
    assert APR.train_group([a, b], epochs=0) == [] and a.epochs_done.tolist() == [0]
    a.eps = float("nan")
    with pytest.raises(ValueError, match="eps"):
        APR.train_group([b, a])
    assert a.epochs_done.tolist() == b.epochs_done.tolist() == [0] and a._steps_done() == 0


def test_train_group_has_no_cpu_fallback():
    with pytest.raises(_lib.HipCallError, match="no CPU fallback"):
        APR.train_group([_apr(), _apr()])


# ------------------------------------------------------------------------------------------------------------ the workflow
def test_sweep_defaults_and_registration():
    cfg = default.WORKFLOW["sweep"]
    plain = default.WORKFLOW["no defense"]
    assert set(cfg) == (set(plain) - {"target_id_list"}) | {"group"}
    assert {k: cfg[k] for k in cfg if k != "group"} == {k: plain[k] for k in cfg if k != "group"}
    assert isinstance(cfg["group"], int) and cfg["group"] >= 1
    assert workflow.factories["sweep"] is workflow.Sweep and issubclass(workflow.Sweep, workflow.Normal)
    assert set(workflow.factories) == {"no defense", "defense", "sweep"}
    ds = _tiny()
    case = {"attacker": workflow.RandomAttack(ds.n_items, seed=1), "target_id_list": [0]}
    for kw in (dict(victim=_StubVictim()), dict(victim_data=ds, attack_data=None, victim=_StubVictim()),
               dict(victim_data=ds, attack_data=None, cases=[case]), dict(victim_data=ds, victim=_StubVictim(), cases=[case])):
        with pytest.raises(TypeError, match="cases"):
            workflow.from_config("sweep", **kw)
    for cases in ([], [{"attacker": case["attacker"]}], [{"target_id_list": [0]}], [dict(case, target_id_list=[])], [case["attacker"]]):
        with pytest.raises(ValueError, match="sweep"):
            workflow.from_config("sweep", victim_data=ds, attack_data=None, victim=_StubVictim(), cases=cases)
    for group in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="group"):
            workflow.from_config("sweep", victim_data=ds, attack_data=None, victim=_StubVictim(), cases=[case], group=group)
    with pytest.raises(ValueError, match="quality_split"):
        workflow.from_config("sweep", victim_data=ds, attack_data=None, victim=_StubVictim(), cases=[case], quality_split="train")
    wf = workflow.from_config("sweep", victim_data=ds, attack_data=None, victim=_StubVictim(), cases=[case], not_a_key=1)
    assert wf.c["group"] == cfg["group"] and "not_a_key" not in wf.c and wf.c["rec_epoch"] == 400


def _cases(ds):
    """three cases told apart by their profile counts; the stub's scores lift item 0 on a poisoned set and leave item 3"""
    return [{"attacker": workflow.RandomAttack(ds.n_items, attack_num=n, filler_num=5, seed=n), "target_id_list": t}
            for n, t in ((10, [0]), (7, [3]), (12, [0]))]


def test_sweep_with_a_victim_without_train_group_retrains_one_after_another():
    ds = _tiny()
    assert not hasattr(_StubVictim, "train_group")
    wf = workflow.from_config("sweep", victim_data=ds, attack_data=None, victim=_StubVictim(), cases=_cases(ds), rec_epoch=2, attack_epoch=0,
                              device=torch.device("cpu"), group=2)
    seen = []
    evaluate = wf.normal_evaluate
    wf.normal_evaluate = lambda model_, fake, *a, **k: (seen.append((model_, fake, a[1])), evaluate(model_, fake, *a, **k))[1]
    res = wf.execute()
    assert isinstance(res, list) and res is wf.results and len(res) == 3
    assert [d.n_users for d in wf.fake_datasets] == [ds.n_users + 10, ds.n_users + 7, ds.n_users + 12], "case order"
    assert [v.dataset for v in wf.fake_victims] == wf.fake_datasets
    per_epoch = sum(1 for _ in ds.generate_batch())
    assert wf.victim.steps == 2 * per_epoch and len(wf.losses) == 2, "the clean victim is trained once"
    assert all(v.steps >= 2 * per_epoch for v in wf.fake_victims) and wf.losses_fake == [[(0.5,), (0.5,)]] * 3
    assert [s[0] for s in seen] == [wf.victim] * 3 and [s[1] for s in seen] == wf.fake_victims and [s[2] for s in seen] == [[0], [3], [0]]
    assert [r["pred_shift"] for r in res] == [pytest.approx(50.0), pytest.approx(0.0), pytest.approx(50.0)]
    for r in res:
        assert set(r) >= {"pred_shift", "HR@10", "HR@10 after attack", "HR@100", "n_eval_users"}
    assert set(wf.timings) == {"train_clean_s", "train_poisoned_s", "evaluate_s"} and len(wf.timings["train_poisoned_s"]) == 2


class _Counting(_StubVictim):
    calls = []

    def I(self, dataset=None, **kw):
        return _Counting(dataset)

    def reset(self, **kw):
        return _Counting()

    @staticmethod
    def train_group(victims, epochs=1, progress_bar=None):
        _Counting.calls.append(len(victims))
        return [[v.train_step(progress_bar=progress_bar, target_id_list=None)[0] for v in victims] for _ in range(epochs)]


@pytest.mark.parametrize("group,calls", [(1, []), (2, [2, 1]), (3, [3]), (8, [3])])
def test_sweep_group_1_never_calls_train_group(group, calls):
    ds = _tiny()
    _Counting.calls = []
    wf = workflow.from_config("sweep", victim_data=ds, attack_data=None, victim=_Counting(), cases=_cases(ds), rec_epoch=2, attack_epoch=0,
                              device=torch.device("cpu"), group=group)
    res = wf.execute()
    assert _Counting.calls == calls and len(wf.timings["train_poisoned_s"]) == max(1, len(calls)) + (2 if group == 1 else 0)
    assert wf.losses_fake == [[(0.5,), (0.5,)]] * 3
    assert [r["pred_shift"] for r in res] == [pytest.approx(50.0), pytest.approx(0.0), pytest.approx(50.0)]
    per_epoch = sum(1 for _ in ds.generate_batch())
    assert wf.victim.steps == 2 * per_epoch, "the clean victim is never in a group"
