from .aush import Aush, RandomAttacker

__all__ = ["Aush", "RandomAttacker"]
