from .apr import APR
from .base import BaseVictim
from .ease import EASE
from .ials import IALS
from .itemknn import ItemKNN
from .lightgcn import LightGCN
from .mf import MF
from .multvae import MultVAE
from .ncf import NCF
from .rp3beta import RP3beta
from .slim import SLIM
from .userknn import UserKNN

__all__ = ["APR", "BaseVictim", "EASE", "IALS", "ItemKNN", "LightGCN", "MF", "MultVAE", "NCF", "RP3beta", "SLIM", "UserKNN"]
