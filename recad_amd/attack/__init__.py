from .aia import AIA
from .aush import Aush, RandomAttacker
from .aushplus import AushPlus

__all__ = ["AIA", "Aush", "AushPlus", "RandomAttacker"]
