from .pca_select_users import PCASelectUsers

__all__ = ["PCASelectUsers"]
