from .catchsync_select_users import CatchSyncSelectUsers
from .fraudar_select_users import FraudarSelectUsers
from .knn_select_users import KnnSelectUsers
from .pca_select_users import PCASelectUsers

__all__ = ["CatchSyncSelectUsers", "FraudarSelectUsers", "KnnSelectUsers", "PCASelectUsers"]
