from .base import BaseVictim
from .itemknn import ItemKNN
from .lightgcn import LightGCN
from .mf import MF
from .ncf import NCF

__all__ = ["BaseVictim", "ItemKNN", "LightGCN", "MF", "NCF"]
