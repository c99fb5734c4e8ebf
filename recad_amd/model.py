"""model.from_config("victim" | "defender", name, **kw): the reference's factory (recad/model/__init__.py:3-21)
for the victims and the defender this build implements."""
from . import defense, victim

factories = {"victim": {"lightgcn": victim.LightGCN, "mf": victim.MF, "ncf": victim.NCF},
             "defender": {"PCASelectUsers": defense.PCASelectUsers}}


def from_config(scope, name, **kwargs):
    return factories[scope][name].from_config(**kwargs)
