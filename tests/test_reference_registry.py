"""INTEGRATION.md option A, executed as far as a machine without a GPU allows: the build's victims registered in a factory
laid out like the reference's (recad/model/__init__.py:3-21: scope -> name -> class, `from_config(scope, name, **kw)` ->
`cls.from_config(**kw)`, lazy `.I(dataset=...)`), instantiated on a foreign dataset object that carries the reference's own
dev graph (tests/golden/lightgcn_dev_d64.npz, recorded from the reference's ImplicitData on its `dev` split), and handed to
the `Normal` workflow constructor.  Training on the CPU device must refuse loudly (no CPU fallback), with or without a GPU
in the machine.  Self-contained: nothing outside the repository is read."""
import numpy as np
import pytest
import torch

from tests import _golden as G
from tests._stub import LGN_KEYS, ReplayDataset


@pytest.fixture(scope="module")
def dev_data():
    g = G.load("lightgcn_dev_d64")
    return g, ReplayDataset(g, LGN_KEYS)


def test_victims_register_in_the_reference_factory(dev_data):
    import recad_amd
    from recad_amd import _lib, model, workflow
    from recad_amd.victim import MF, NCF, LightGCN
    g, ds = dev_data
    saved = dict(model.factories["victim"])
    try:
        model.factories["victim"].clear()
        model.factories["victim"].update({"lightgcn": LightGCN, "mf": MF, "ncf": NCF})
        lazy = model.from_config("victim", "lightgcn", latent_dim_rec=32)
        assert isinstance(lazy, LightGCN) and lazy.model_name == "lightgcn"
        with pytest.raises(recad_amd.utils.NotInstantiatedError):
            lazy.train_step()
        m = lazy.I(dataset=ds)                                                          # a dataset object the build did not make
        info = ds.info_describe()
        assert (info["n_users"], info["n_items"]) == (int(g["n_users"]), int(g["n_items"])) == (512, 511)
        assert tuple(m.embedding_user.weight.shape) == (info["n_users"], 32)
        assert tuple(m.embedding_item.weight.shape) == (info["n_items"], 32)
        assert m.Graph.shape == (info["n_users"] + info["n_items"],) * 2 and m.Graph.is_sparse      # implicit.py:320-326
        assert np.array_equal(m.Graph.coalesce().indices().numpy(), info["graph"].indices().numpy())
        assert set(m.input_describe()["forward"]) == {"users", "items"}                # normal.py:122-131
        assert len(m.output_describe()["train_step"]) == 1
        assert isinstance(m.reset(), LightGCN)
        # the workflow object accepts it (normal.py:25-40); running it needs the device
        attacker = workflow.RandomAttack(info["n_items"], seed=2)
        wf = workflow.from_config("no defense", victim_data=ds, attack_data=None, victim=model.from_config("victim", "lightgcn"),
                                  attacker=attacker, rec_epoch=1, attack_epoch=0, device=torch.device("cpu"))
        assert isinstance(wf.victim, LightGCN) and wf.victim.embedding_user.weight.shape[0] == info["n_users"]
        with pytest.raises(_lib.HipCallError):        # no CPU fallback: the path fails loudly without its HIP device
            wf.execute()
        for name, cls in (("mf", MF), ("ncf", NCF)):
            v = model.from_config("victim", name).I(dataset=ds)
            assert isinstance(v, cls) and set(v.input_describe()["train_step"]) == {"users", "items", "labels"}
    finally:
        model.factories["victim"].clear()
        model.factories["victim"].update(saved)
