from .base import BaseVictim
from .ease import EASE
from .ials import IALS
from .itemknn import ItemKNN
from .lightgcn import LightGCN
from .mf import MF
from .ncf import NCF

__all__ = ["BaseVictim", "EASE", "IALS", "ItemKNN", "LightGCN", "MF", "NCF"]
