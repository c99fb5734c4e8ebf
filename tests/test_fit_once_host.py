"""CPU tests of what the fit-once victims (ItemKNN, RP3beta, EASE, SLIM) take from their common base
(recad_amd/victim/_fit_once.py): the lazy-init guard on the inherited methods, the refusal to run on the CPU, and the keys of
the state."""
import pytest
import torch

from recad_amd import _lib, dataset, model, synth
from recad_amd.utils import NotInstantiatedError
from recad_amd.victim._fit_once import FitOnceVictim

STATE = {"itemknn": {"nbr_w", "nbr_id", "fitted"}, "rp3beta": {"nbr_w", "nbr_id", "fitted"}, "ease": {"B", "fitted"},
         "slim": {"W", "fitted"}}


def _tiny():
    d = synth.make("tiny")
    return dataset.from_config("implicit", "tiny", train_csr=d["train"], valid_csr=d["valid"], test_csr=d["test"],
                               need_graph=False, device=torch.device("cpu"), seed=5)


@pytest.mark.parametrize("name", sorted(STATE))
def test_inherited_methods_keep_the_contract(name):
    lazy = model.from_config("victim", name)
    assert isinstance(lazy, FitOnceVictim)
    for call in (lazy.fit, lazy.train_step, lambda: lazy.forward(None, None), lambda: lazy.score_matrix(None, None),
                 lazy.input_describe):
        with pytest.raises(NotInstantiatedError):
            call()
    real = lazy.I(dataset=_tiny())
    with pytest.raises(_lib.HipCallError, match="no CPU fallback"):
        real.train_step()
    assert set(real.state_dict()) == STATE[name] and real.fitted.tolist() == [0]
