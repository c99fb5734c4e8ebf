from .aia import AIA
from .aush import Aush, RandomAttacker

__all__ = ["AIA", "Aush", "RandomAttacker"]
