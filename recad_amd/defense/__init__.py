from .catchsync_select_users import CatchSyncSelectUsers
from .knn_select_users import KnnSelectUsers
from .pca_select_users import PCASelectUsers

__all__ = ["CatchSyncSelectUsers", "KnnSelectUsers", "PCASelectUsers"]
