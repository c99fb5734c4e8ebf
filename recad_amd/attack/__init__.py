from .aia import AIA
from .aush import Aush, RandomAttacker
from .aushplus import AushPlus
from .heuristic import AverageAttack, BandwagonAttack, SegmentAttack
from .pga import PGA
from .uba import UBA

__all__ = ["AIA", "Aush", "AushPlus", "AverageAttack", "BandwagonAttack", "PGA", "RandomAttacker", "SegmentAttack", "UBA"]
