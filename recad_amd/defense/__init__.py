from .knn_select_users import KnnSelectUsers
from .pca_select_users import PCASelectUsers

__all__ = ["KnnSelectUsers", "PCASelectUsers"]
