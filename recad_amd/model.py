"""model.from_config("victim" | "attacker" | "defender", name, **kw): the reference's factory (recad/model/__init__.py:3-21)
for the victims, attackers and defenders this build implements."""
from . import attack, defense, victim

factories = {"victim": {"lightgcn": victim.LightGCN, "mf": victim.MF, "ncf": victim.NCF,
                        "itemknn": victim.ItemKNN, "ease": victim.EASE, "ials": victim.IALS, "slim": victim.SLIM, "apr": victim.APR,
                        "multvae": victim.MultVAE, "rp3beta": victim.RP3beta, "userknn": victim.UserKNN},
             "attacker": {"aia": attack.AIA, "aush": attack.Aush, "aushplus": attack.AushPlus, "random": attack.RandomAttacker,
                          "average": attack.AverageAttack, "segment": attack.SegmentAttack, "bandwagon": attack.BandwagonAttack,
                          "uba": attack.UBA, "pga": attack.PGA},
             "defender": {"PCASelectUsers": defense.PCASelectUsers, "KnnSelectUsers": defense.KnnSelectUsers,
                          "CatchSyncSelectUsers": defense.CatchSyncSelectUsers, "FraudarSelectUsers": defense.FraudarSelectUsers}}


def from_config(scope, name, **kwargs):
    return factories[scope][name].from_config(**kwargs)
