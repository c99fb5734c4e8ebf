"""CPU tests of SelectUsersDefender, the base of the four defenders: what the subclasses no longer define, the lazy guard on
what they inherit, the order of a step's calls with the state it leaves, and the shared _flag / _pairs / flag_count."""
import numpy as np
import pytest
import torch

from recad_amd import _lib, defense, model
from recad_amd.defense import _select_users as base
from recad_amd.defense._select_users import SelectUsersDefender, flag_count
from recad_amd.utils import NotInstantiatedError

DEFENDERS = [defense.PCASelectUsers, defense.KnnSelectUsers, defense.CatchSyncSelectUsers, defense.FraudarSelectUsers]
SHARED = ("_shape", "forward", "train_step", "input_describe", "output_describe", "defense_step")


class _Described:
    def __init__(self, n_users, n_items):
        self.shape = (n_users, n_items)

    def info_describe(self):
        return {"n_users": self.shape[0], "n_items": self.shape[1], "train_mat": None}


class Stub(SelectUsersDefender):
    def _build(self, attack_num, refuse=False, log=None, **config):
        self.attack_num, self.refuse, self.predLabels = int(attack_num), refuse, None
        self.calls = [] if log is None else log             # the fixture's log, so that one list holds the order of all calls
        self._open(config)

    def _check(self):
        self.calls.append("check")
        if self.refuse:
            raise ValueError("Stub: refused on the host")

    def _detect(self, U, I, rowptr, col, val):
        self.calls.append(("detect", U, I, self.user_num, self.item_num))
        return self._flag(torch.arange(U - 1, -1, -1, dtype=torch.int32), U)


@pytest.fixture
def traced(monkeypatch):
    """require_gpu and the base module's rating_csr replaced by recorders: (datasets seen by rating_csr, the shared call log)."""
    log, seen = [], []

    def rating_csr(dataset, device):
        log.append("rating_csr")
        seen.append(dataset)
        U, I = dataset.shape if hasattr(dataset, "shape") else (len(dataset[0]) - 1, 9)
        return U, I, None, None, None

    monkeypatch.setattr(_lib, "require_gpu", lambda: log.append("require_gpu"))
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("a stub step needs no library"))
    monkeypatch.setattr(base, "rating_csr", rating_csr)
    return seen, log


@pytest.mark.parametrize("cls", DEFENDERS)
def test_the_defenders_keep_only_what_is_theirs(cls):
    assert issubclass(cls, SelectUsersDefender) and cls.scope == "defender"
    assert model.from_config("defender", cls.victim_name).__class__ is cls
    assert not [name for name in SHARED if name in cls.__dict__]
    assert "_detect" in cls.__dict__ and "_build" in cls.__dict__


@pytest.mark.parametrize("cls", DEFENDERS)
def test_inherited_methods_are_guarded_on_a_lazy_instance(cls):
    lazy = model.from_config("defender", cls.victim_name)
    with pytest.raises(NotInstantiatedError, match="defense_step"):
        lazy.defense_step()
    with pytest.raises(NotInstantiatedError, match="input_describe"):
        lazy.input_describe()
    built = lazy.I(dataset=None)
    assert built.input_describe() == {"defense_step": {"dataset": (object, [])}}
    assert built.output_describe() == {"defense_step": {"spam_list": (list, [])}}
    assert built.forward() is None and built.train_step() is None
    assert built.user_num is None and built.item_num is None and built.predLabels is None
    assert built.logger.name == cls.__module__


def test_a_step_calls_in_order_and_refreshes_the_shape(traced):
    seen, log = traced
    first, second = np.ones((6, 4)), np.ones((8, 5))
    d = Stub(attack_num=3, log=log).I(dataset=first)
    assert (d.user_num, d.item_num) == (6, 4) and d.device == torch.device("cuda")
    assert d.defense_step() == [5, 4, 3]
    assert log == ["check", "require_gpu", "rating_csr", ("detect", 6, 4, 6, 4)] and seen == [first]
    del log[:]
    assert d.defense_step(dataset=second) == [7, 6, 5]          # the step's dataset replaces the one given to .I()
    assert log == ["check", "require_gpu", "rating_csr", ("detect", 8, 5, 8, 5)] and seen[-1] is second and d.dataset is second
    assert (d.user_num, d.item_num) == (8, 5)


def test_refusals_come_before_the_device(traced):
    _, log = traced
    d = Stub(attack_num=3, log=log).I()
    assert d.dataset is None and d.user_num is None and d.item_num is None
    with pytest.raises(ValueError, match=r"^Stub\.defense_step: no dataset \(give one to \.I\(\) or to defense_step\)$"):
        d.defense_step()
    assert log == ["check"]                                     # the host check ran, the device was not asked
    d = Stub(attack_num=3, refuse=True, log=log).I(dataset=np.ones((2, 2)))
    with pytest.raises(ValueError, match="refused on the host"):
        d.defense_step()
    d = Stub(attack_num=3, refuse=True, log=log).I()
    with pytest.raises(ValueError, match="refused on the host"):  # and it goes before the missing dataset
        d.defense_step()
    assert log == ["check"] * 3


def test_the_three_kinds_of_dataset(traced):
    ptr, idx, val = np.array([0, 2, 3, 3]), np.array([0, 8, 1]), np.ones(3, dtype=np.float32)
    d = Stub(attack_num=1).I(dataset=_Described(7, 3))
    assert (d.user_num, d.item_num) == (7, 3)
    d = Stub(attack_num=1).I(dataset=(ptr, idx, val, 12))
    assert (d.user_num, d.item_num) == (3, 12)
    d = Stub(attack_num=1).I(dataset=(ptr, idx, val))
    assert (d.user_num, d.item_num) == (3, None)                # a 3-tuple does not say how many items there are
    assert d.defense_step() == [2] and (d.user_num, d.item_num) == (3, 9)
    d = Stub(attack_num=1).I(dataset=torch.ones(4, 2))
    assert (d.user_num, d.item_num) == (4, 2)


def test_flag_and_pairs():
    d = Stub(attack_num=2).I()
    assert d._pairs(torch.zeros(5)) is None                      # nothing ranked yet
    order = torch.tensor([3, 0, 4, 1, 2], dtype=torch.int32)
    values = torch.tensor([0.5, 0.25, 2.0, 0.125, 1.0], dtype=torch.float32)
    assert d._flag(order, 5) == [3, 0] and flag_count(2, 5) == 2
    assert d.predLabels.tolist() == [1, 0, 0, 1, 0] and d.predLabels.dtype == np.float64
    pairs = d._pairs(values)
    assert pairs == [(3, 0.125), (0, 0.5), (4, 1.0), (1, 0.25), (2, 2.0)] and all(type(v) is float for _, v in pairs)
    assert d._pairs(values * 2) is pairs                         # built once
    assert d._flag(order.flip(0), 5) == [2, 1] and d._pairs(values)[0] == (2, 2.0)   # a new step, a new list


def test_flag_count_values():
    """What flag_count gave before it moved here; both homes hold the one function."""
    from recad_amd.defense import pca_select_users

    assert (flag_count(7, 49), flag_count(0, 10), flag_count(99, 10)) == (7, 0, 10)
    assert pca_select_users.flag_count is flag_count and callable(pca_select_users.rating_csr)
